/**
 * @file swing_tests.cpp
 * Tests of the Planners::SwingFootPlanner and Planners::SO3Planner adapters, with host_tests.cpp's
 * conventions ("name ... ok", "N checks, 0 failed"; modes cpu / gpu / all):
 *   cpu: every path on which the adapters return false without touching a device (parameter
 *        handler errors, setContactList before initialize, an empty list, SO3Planner misuse);
 *   gpu: a two-contact list walked by advance() equals blf_swing_foot_eval sample for sample,
 *        isInContact flips at the lift and landing samples, advance() returns false at the end,
 *        and SO3Planner::evaluatePoint equals blf_so3_eval.
 */
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include <BipedalLocomotion/ParametersHandler/IParametersHandler.h>
#include <BipedalLocomotion/Planners/SO3Planner.h>
#include <BipedalLocomotion/Planners/SwingFootPlanner.h>

#include "test_harness.h"

using namespace BipedalLocomotion::Planners;
using namespace BipedalLocomotion::ParametersHandler;

static const double kDT = 0.0625, kHeight = 0.05, kApex = 0.4, kVland = -0.02, kAland = 0.1;

static std::shared_ptr<StdImplementation> handlerWithout(const std::string& key)
{
    auto h = std::make_shared<StdImplementation>();
    if (key != "sampling_time") h->setParameter("sampling_time", kDT);
    if (key != "step_height") h->setParameter("step_height", kHeight);
    if (key != "foot_apex_time") h->setParameter("foot_apex_time", kApex);
    if (key != "foot_landing_velocity") h->setParameter("foot_landing_velocity", kVland);
    if (key != "foot_landing_acceleration") h->setParameter("foot_landing_acceleration", kAland);
    return h;
}

static ContactList twoContacts()
{
    ContactList list;
    Contact a, b;
    a.pose = blf::Transform::fromPlanar(0.0, 0.1, 0.05);
    a.activationTime = 0.0;
    a.deactivationTime = 0.5;
    b.pose = blf::Transform::fromPlanar(0.3, 0.12, -0.08, 0.02);
    b.activationTime = 1.0;
    b.deactivationTime = 2.0;
    list.addContact(a);
    list.addContact(b);
    return list;
}

static void testParameterHandler()
{
    {
        SwingFootPlanner planner;
        std::weak_ptr<IParametersHandler> expired;
        {
            auto temporary = handlerWithout("");
            expired = temporary;
        }
        REQUIRE_FALSE(planner.initialize(expired));
        REQUIRE_FALSE(planner.isValid());
        REQUIRE(planner.initialize(handlerWithout("")));
    }
    for (const char* key : {"sampling_time", "step_height", "foot_apex_time"})
    {
        SwingFootPlanner planner;
        REQUIRE_FALSE(planner.initialize(handlerWithout(key)));
    }
    for (const char* key : {"foot_landing_velocity", "foot_landing_acceleration"})
    {
        SwingFootPlanner planner;   // optional keys
        REQUIRE(planner.initialize(handlerWithout(key)));
    }
    const struct { const char* key; double value; } bad[] = {
        {"sampling_time", 0.0}, {"sampling_time", -0.01}, {"step_height", -0.01},
        {"foot_apex_time", 0.0}, {"foot_apex_time", 1.0}, {"foot_apex_time", 1.5},
        {"foot_landing_velocity", INFINITY}, {"foot_landing_acceleration", NAN}};
    for (const auto& b : bad)
    {
        auto h = handlerWithout("");
        h->setParameter(b.key, b.value);
        SwingFootPlanner planner;
        REQUIRE_FALSE(planner.initialize(h));
    }
}

static void testStateMachine()
{
    {
        SwingFootPlanner planner;   // setContactList and advance before initialize
        REQUIRE_FALSE(planner.setContactList(twoContacts()));
        REQUIRE_FALSE(planner.advance());
        REQUIRE_FALSE(planner.isValid());
    }
    {
        SwingFootPlanner planner;   // an empty list, a list too long; advance without a list
        REQUIRE(planner.initialize(handlerWithout("")));
        REQUIRE_FALSE(planner.setContactList(ContactList()));
        ContactList longList;
        for (int i = 0; i < BLF_SWING_MAX_CONTACTS + 1; ++i)
            REQUIRE(longList.addContact(blf::Transform::Identity(), 2.0 * i, 2.0 * i + 1.0));
        REQUIRE_FALSE(planner.setContactList(longList));
        REQUIRE_FALSE(planner.advance());
        REQUIRE_FALSE(planner.isValid());
    }
    {
        SO3Planner so3;
        blf::Matrix3 R{};
        blf::Vector3 w{}, a{};
        REQUIRE_FALSE(so3.evaluatePoint(0.0, R, w, a));   // before setRotations
        const blf::Matrix3 I = blf::Transform::Identity().rotation;
        REQUIRE_FALSE(so3.setRotations(I, I, 0.0));
        REQUIRE_FALSE(so3.setRotations(I, I, -1.0));
        REQUIRE_FALSE(so3.setRotations(I, I, NAN));
        REQUIRE(so3.setRotations(I, I, 2.0));
        REQUIRE_FALSE(so3.evaluatePoint(-0.1, R, w, a));  // outside [0, duration]
        REQUIRE_FALSE(so3.evaluatePoint(2.1, R, w, a));
        REQUIRE_FALSE(so3.evaluatePoint(NAN, R, w, a));
    }
}

static void testSwingFootPlannerOnDevice()
{
    const ContactList list = twoContacts();
    SwingFootPlanner planner;
    REQUIRE(planner.initialize(handlerWithout("")));
    REQUIRE(planner.setContactList(list));
    REQUIRE(planner.isValid());

    // the same samples straight through the C ABI
    const std::size_t K = 17;   // t = 0, 1/16, ..., 1
    std::vector<double> host(2 * 12 + 2 * 2 + K);
    const auto pa = list[0].pose.packed(), pb = list[1].pose.packed();
    std::copy(pa.begin(), pa.end(), host.begin());
    std::copy(pb.begin(), pb.end(), host.begin() + 12);
    const double times[4] = {0.0, 0.5, 1.0, 2.0};
    std::copy(times, times + 4, host.begin() + 24);
    for (std::size_t k = 0; k < K; ++k) host[28 + k] = 0.0 + static_cast<double>(k) * kDT;
    blf::DeviceBuffer<double> in, out(K * 24);
    blf::DeviceBuffer<int32_t> ints;
    REQUIRE(in.upload(host));
    REQUIRE(ints.upload(std::vector<int32_t>(1 + K, 2)));
    blf_swing_foot_params prm{2, 0, kHeight, kApex, kVland, kAland};
    REQUIRE(blf_swing_foot_eval(blf::threadHandle(), &prm, in.data(), in.data() + 24, ints.data(), 1,
                                in.data() + 28, static_cast<int32_t>(K), out.data(),
                                out.data() + K * 12, out.data() + K * 18, nullptr, ints.data() + 1,
                                nullptr) == BLF_OK);
    std::vector<double> ref;
    std::vector<int32_t> refInt;
    REQUIRE(out.download(ref));
    REQUIRE(ints.download(refInt));

    std::size_t k = 0;
    bool more = true;
    while (more && k < K)
    {
        const SwingFootPlannerState& s = planner.get();
        const auto pose = s.transform.packed();
        REQUIRE(std::memcmp(pose.data(), ref.data() + k * 12, 12 * sizeof(double)) == 0);
        REQUIRE(std::memcmp(s.mixedVelocity.data(), ref.data() + K * 12 + k * 6, 6 * sizeof(double)) == 0);
        REQUIRE(std::memcmp(s.mixedAcceleration.data(), ref.data() + K * 18 + k * 6, 6 * sizeof(double)) == 0);
        REQUIRE(s.isInContact == (refInt[1 + k] != 0));
        REQUIRE(s.time == host[28 + k]);
        // in contact up to the lift sample (t = 0.5, k = 8) exclusive, again from the landing
        // sample (t = 1, k = 16)
        REQUIRE(s.isInContact == (k < 8 || k == 16));
        if (k > 8 && k < 16) REQUIRE(s.transform.position[2] > 0.0);
        more = planner.advance();
        ++k;
    }
    REQUIRE(k == K);          // 17 samples ...
    REQUIRE_FALSE(more);      // ... and advance() is false past the last contact's activation
    REQUIRE(planner.get().time == 1.0);
    REQUIRE(planner.isValid());
    const auto last = planner.get().transform.packed();
    REQUIRE(std::memcmp(last.data(), pb.data(), sizeof(pb)) == 0);

    // a new list restarts the walk
    REQUIRE(planner.setContactList(list));
    REQUIRE(planner.get().time == 0.0);
    REQUIRE(planner.advance());
}

static void testSO3PlannerOnDevice()
{
    const blf::Matrix3 R0 = blf::Transform::fromPlanar(0.0, 0.0, 0.3).rotation;
    // a rotation about x by 1.2 rad after R0
    const double c = std::cos(1.2), s = std::sin(1.2);
    const blf::Matrix3 Rx{{1.0, 0.0, 0.0, 0.0, c, -s, 0.0, s, c}};
    blf::Matrix3 R1{};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            R1[3 * i + j] = Rx[3 * i] * R0[j] + Rx[3 * i + 1] * R0[3 + j] + Rx[3 * i + 2] * R0[6 + j];
    const double T = 1.5;
    SO3Planner so3;
    REQUIRE(so3.setRotations(R0, R1, T));

    const std::vector<double> tq{0.0, 0.3, 0.75, 1.2, 1.5};
    std::vector<double> host(20 + tq.size());
    std::copy(R0.begin(), R0.end(), host.begin());
    std::copy(R1.begin(), R1.end(), host.begin() + 9);
    host[18] = T;
    std::copy(tq.begin(), tq.end(), host.begin() + 20);
    blf::DeviceBuffer<double> in, out(tq.size() * 15);
    REQUIRE(in.upload(host));
    const int32_t Q = static_cast<int32_t>(tq.size());
    REQUIRE(blf_so3_eval(blf::threadHandle(), in.data(), in.data() + 9, in.data() + 18, 1,
                         in.data() + 20, Q, out.data(), out.data() + Q * 9, out.data() + Q * 12,
                         nullptr) == BLF_OK);
    std::vector<double> ref;
    REQUIRE(out.download(ref));
    for (std::size_t q = 0; q < tq.size(); ++q)
    {
        blf::Matrix3 R{};
        blf::Vector3 w{}, a{};
        REQUIRE(so3.evaluatePoint(tq[q], R, w, a));
        REQUIRE(std::memcmp(R.data(), ref.data() + q * 9, 9 * sizeof(double)) == 0);
        REQUIRE(std::memcmp(w.data(), ref.data() + Q * 9 + q * 3, 3 * sizeof(double)) == 0);
        REQUIRE(std::memcmp(a.data(), ref.data() + Q * 12 + q * 3, 3 * sizeof(double)) == 0);
    }
    blf::Matrix3 R{};
    blf::Vector3 w{}, a{};
    REQUIRE(so3.evaluatePoint(0.0, R, w, a));
    REQUIRE(R == R0);                                   // s = 0: R0 bit for bit
    REQUIRE(so3.evaluatePoint(T, R, w, a));
    for (int i = 0; i < 9; ++i) REQUIRE(std::abs(R[i] - R1[i]) < 1e-13);
    REQUIRE(so3.evaluatePoint(0.5 * T, R, w, a));
    REQUIRE(std::abs(w[0] - 1.875 * 1.2 / T) < 1e-12);  // the peak rate, about x
    REQUIRE(std::abs(w[1]) < 1e-12 && std::abs(w[2]) < 1e-12);
}

int main(int argc, char** argv)
{
    return runCases(argc, argv, {
        {"SwingFootPlanner parameter handler", false, testParameterHandler},
        {"SwingFootPlanner state machine", false, testStateMachine},
        {"SwingFootPlanner on the device", true, testSwingFootPlannerOnDevice},
        {"SO3Planner on the device", true, testSO3PlannerOnDevice},
    });
}
