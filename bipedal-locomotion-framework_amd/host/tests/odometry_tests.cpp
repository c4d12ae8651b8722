/**
 * @file odometry_tests.cpp
 * Tests of the Contacts::SchmittTriggerDetector and Estimators::LeggedOdometry adapters, with
 * host_tests.cpp's conventions ("name ... ok", "N checks, 0 failed"; modes cpu / gpu / all):
 *   cpu: the state machines and every path on which an adapter returns false without touching a device;
 *   gpu: a two-foot walk of six steps on ik_fixtures.h's 13-joint biped through the two adapters (the
 *        detector's contacts handed to the odometry with setContactStatus) against
 *        blf_legged_odometry_advance called directly on the same samples with its own triggers: the same
 *        base pose and twist bit for bit, the same fixed frame; then changeFixedFrame.
 */
#include <cmath>
#include <cstdio>
#include <memory>
#include <string>
#include <vector>

#include <BipedalLocomotion/ContactDetectors/SchmittTriggerDetector.h>
#include <BipedalLocomotion/FloatingBaseEstimators/LeggedOdometry.h>
#include <BipedalLocomotion/ParametersHandler/IParametersHandler.h>

#include "ik_fixtures.h"
#include "test_harness.h"

using namespace BipedalLocomotion::Contacts;
using namespace BipedalLocomotion::Estimators;
using namespace BipedalLocomotion::ParametersHandler;

static const std::vector<std::string> kSoles = {"l_sole", "r_sole"};

static std::shared_ptr<StdImplementation> detectorHandler(const std::string& without = "")
{
    auto h = std::make_shared<StdImplementation>();
    if (without != "contacts") h->setParameter("contacts", kSoles);
    if (without != "contact_make_thresholds") h->setParameter("contact_make_thresholds", std::vector<double>{10.0, 10.0});
    if (without != "contact_break_thresholds") h->setParameter("contact_break_thresholds", std::vector<double>{4.0, 4.0});
    if (without != "contact_make_switch_times") h->setParameter("contact_make_switch_times", std::vector<double>{0.0, 0.0});
    if (without != "contact_break_switch_times") h->setParameter("contact_break_switch_times", std::vector<double>{0.0, 0.0});
    return h;
}

static std::shared_ptr<StdImplementation> odometryHandler(const std::string& frame = "l_sole")
{
    auto h = std::make_shared<StdImplementation>();
    h->setParameter("initial_fixed_frame", frame);
    return h;
}

static void testDetectorStateMachine()
{
    EstimatedContact c;
    {   // everything before initialize
        SchmittTriggerDetector d;
        REQUIRE_FALSE(d.advance());
        REQUIRE_FALSE(d.setTimedTriggerInput("l_sole", 0.0, 1.0));
        REQUIRE_FALSE(d.resetContact("l_sole", true));
        REQUIRE_FALSE(d.get("l_sole", c));
        REQUIRE(d.getOutput().empty());
    }
    {   // a second initialize, an expired handler, each missing key
        SchmittTriggerDetector d;
        REQUIRE(d.initialize(detectorHandler()));
        REQUIRE_FALSE(d.initialize(detectorHandler()));
        SchmittTriggerDetector e;
        std::weak_ptr<IParametersHandler> expired;
        {
            auto temporary = detectorHandler();
            expired = temporary;
        }
        REQUIRE_FALSE(e.initialize(expired));
        for (const char* key : {"contacts", "contact_make_thresholds", "contact_break_thresholds",
                                "contact_make_switch_times", "contact_break_switch_times"})
            REQUIRE_FALSE(e.initialize(detectorHandler(key)));
        REQUIRE(e.initialize(detectorHandler()));
    }
    {   // sizes and values the trigger call refuses
        auto bad = [](const char* key, std::vector<double> v) {
            auto h = detectorHandler();
            h->setParameter(key, v);
            SchmittTriggerDetector d;
            return d.initialize(h);
        };
        REQUIRE_FALSE(bad("contact_make_thresholds", {10.0}));
        REQUIRE_FALSE(bad("contact_make_thresholds", {10.0, 3.0}));           // below the break threshold
        REQUIRE_FALSE(bad("contact_break_thresholds", {4.0, std::nan("")}));
        REQUIRE_FALSE(bad("contact_make_switch_times", {-0.1, 0.0}));
        REQUIRE_FALSE(bad("contact_break_switch_times", {0.0, INFINITY}));
        auto h = detectorHandler();
        h->setParameter("contacts", std::vector<std::string>{"l_sole", "l_sole"});
        SchmittTriggerDetector d;
        REQUIRE_FALSE(d.initialize(h));
        auto many = std::make_shared<StdImplementation>();
        std::vector<std::string> names;
        for (int i = 0; i < 9; ++i) names.push_back("c" + std::to_string(i));
        many->setParameter("contacts", names);
        for (const char* key : {"contact_make_thresholds", "contact_break_thresholds", "contact_make_switch_times",
                                "contact_break_switch_times"})
            many->setParameter(key, std::vector<double>(9, 1.0));
        REQUIRE_FALSE(d.initialize(many));
        auto none = detectorHandler();
        none->setParameter("contacts", std::vector<std::string>{});
        REQUIRE_FALSE(d.initialize(none));
    }
    {   // inputs: unknown names, no input, two clocks in one advance
        SchmittTriggerDetector d;
        REQUIRE(d.initialize(detectorHandler()));
        REQUIRE(d.getOutput().size() == 2);
        REQUIRE(d.get("r_sole", c) && !c.isActive && c.switchTime == 0.0);
        REQUIRE_FALSE(d.get("sole", c));
        REQUIRE_FALSE(d.setTimedTriggerInput("sole", 0.0, 1.0));
        REQUIRE_FALSE(d.resetContact("sole", true));
        REQUIRE_FALSE(d.advance());
        REQUIRE(d.setTimedTriggerInput("l_sole", 0.1, 20.0));
        REQUIRE(d.setTimedTriggerInput("r_sole", 0.2, 20.0));
        REQUIRE_FALSE(d.advance());
        REQUIRE(d.resetContact("l_sole", true, 0.05));
        REQUIRE(d.get("l_sole", c) && c.isActive && c.switchTime == 0.05 && c.lastUpdateTime == 0.05);
    }
}

static void testOdometryStateMachine()
{
    {   // everything before initialize
        LeggedOdometry o;
        REQUIRE_FALSE(o.setRobotModel(bipedModel(), kSoles));
        REQUIRE_FALSE(o.setKinematics(std::vector<double>(kJoints, 0.0), std::vector<double>(kJoints, 0.0)));
        REQUIRE_FALSE(o.setContactStatus("l_sole", true, 0.0, 0.0));
        REQUIRE_FALSE(o.resetEstimator(blf::Transform::Identity()));
        REQUIRE_FALSE(o.changeFixedFrame("l_sole"));
        REQUIRE_FALSE(o.advance());
        REQUIRE(o.getFixedFrameIdx() == -1);
    }
    {   // initialize: twice, expired, the missing key
        LeggedOdometry o;
        REQUIRE_FALSE(o.initialize(std::make_shared<StdImplementation>()));
        std::weak_ptr<IParametersHandler> expired;
        {
            auto temporary = odometryHandler();
            expired = temporary;
        }
        REQUIRE_FALSE(o.initialize(expired));
        REQUIRE(o.initialize(odometryHandler()));
        REQUIRE_FALSE(o.initialize(odometryHandler()));
        // initialised, no model yet
        REQUIRE_FALSE(o.setKinematics(std::vector<double>(kJoints, 0.0), std::vector<double>(kJoints, 0.0)));
        REQUIRE_FALSE(o.setContactStatus("l_sole", true, 0.0, 0.0));
        REQUIRE_FALSE(o.advance());
        REQUIRE_FALSE(o.changeFixedFrame("r_sole"));
    }
    {   // models refused before any device work
        LeggedOdometry o;
        REQUIRE(o.initialize(odometryHandler()));
        blf::RobotModel m = bipedModel();
        m.jointAxis.pop_back();
        REQUIRE_FALSE(o.setRobotModel(m, kSoles));
        m = bipedModel();
        m.parent[3] = 7;
        REQUIRE_FALSE(o.setRobotModel(m, kSoles));
        m = bipedModel();
        m.jointType.assign(kJoints, BLF_JOINT_REVOLUTE);
        m.jointType[2] = 5;
        REQUIRE_FALSE(o.setRobotModel(m, kSoles));
        m = bipedModel();
        m.frameLink[1] = 99;
        REQUIRE_FALSE(o.setRobotModel(m, kSoles));
        m = bipedModel();
        m.frameLink.clear();
        m.framePose.clear();
        REQUIRE_FALSE(o.setRobotModel(m, {}));
        m = bipedModel();
        for (int f = 0; f < 8; ++f)
        {
            m.frameLink.push_back(1);
            m.framePose.insert(m.framePose.end(), {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1});
        }
        REQUIRE_FALSE(o.setRobotModel(m, {}));                                   // ten frames
        REQUIRE_FALSE(o.setRobotModel(bipedModel(), {"l_sole"}));               // one name for two frames
        REQUIRE_FALSE(o.setRobotModel(bipedModel(), {"left", "right"}));        // no frame named l_sole
        REQUIRE_FALSE(o.setRobotModel(bipedModel(), {}));                       // default names are "0", "1"
        REQUIRE(o.getFixedFrameIdx() == -1);
    }
}

static bool same(const double* a, const double* b, int n)
{
    for (int i = 0; i < n; ++i)
        if (!(a[i] == b[i])) return false;
    return true;
}

static void testWalkAgainstTheCAbi()
{
    constexpr int T = 6, K = 2, n = kJoints;
    const double fl[T] = {20.0, 20.0, 20.0, 0.0, 0.0, 0.0}, fr[T] = {0.0, 0.0, 20.0, 20.0, 20.0, 20.0};
    std::vector<double> time(T), q(T * n), dq(T * n), force(T * K);
    for (int t = 0; t < T; ++t)
    {
        time[t] = 0.01 * (t + 1);
        for (int j = 0; j < n; ++j)
        {
            q[t * n + j] = 0.1 * std::sin(0.7 * j + 0.3 * t);
            dq[t * n + j] = 0.2 * std::cos(0.4 * j - 0.5 * t);
        }
        force[t * K] = fl[t];
        force[t * K + 1] = fr[t];
    }
    // through the adapters, one sample at a time
    SchmittTriggerDetector det;
    REQUIRE(det.initialize(detectorHandler()));
    REQUIRE(det.resetContact("l_sole", true, 0.0));
    LeggedOdometry odo;
    REQUIRE(odo.initialize(odometryHandler()));
    REQUIRE(odo.setRobotModel(bipedModel(), kSoles));
    REQUIRE(odo.getFixedFrameIdx() == 0);
    REQUIRE_FALSE(odo.advance());                                   // no kinematics yet
    REQUIRE_FALSE(odo.setKinematics(std::vector<double>(n - 1, 0.0), std::vector<double>(n, 0.0)));
    REQUIRE_FALSE(odo.setContactStatus("sole", true, 0.0, 0.0));
    REQUIRE_FALSE(odo.setContactStatus("l_sole", true, NAN, 0.0));
    REQUIRE_FALSE(odo.changeFixedFrame("r_sole"));                  // no estimate yet
    std::vector<double> pos(T * 3), rot(T * 9), vel(T * 6);
    std::vector<int> fixed(T);
    for (int t = 0; t < T; ++t)
    {
        REQUIRE(det.setTimedTriggerInput("l_sole", time[t], fl[t]));
        REQUIRE(det.setTimedTriggerInput("r_sole", time[t], fr[t]));
        REQUIRE(det.advance());
        for (const auto& name : kSoles)
        {
            EstimatedContact c;
            REQUIRE(det.get(name, c));
            REQUIRE(c.lastUpdateTime == time[t]);
            REQUIRE(odo.setContactStatus(name, c.isActive, c.switchTime, time[t]));
        }
        REQUIRE(odo.setKinematics(std::vector<double>(q.begin() + t * n, q.begin() + (t + 1) * n),
                                  std::vector<double>(dq.begin() + t * n, dq.begin() + (t + 1) * n)));
        REQUIRE(odo.advance());
        const auto& out = odo.getOutput();
        for (int k = 0; k < 3; ++k) pos[3 * t + k] = out.basePose.position[k];
        for (int k = 0; k < 9; ++k) rot[9 * t + k] = out.basePose.rotation[k];
        for (int k = 0; k < 6; ++k) vel[6 * t + k] = out.baseTwist[k];
        fixed[t] = odo.getFixedFrameIdx();
    }
    REQUIRE((fixed == std::vector<int>{0, 0, 0, 1, 1, 1}));
    EstimatedContact c;
    REQUIRE(det.get("l_sole", c) && !c.isActive && c.switchTime == time[3]);
    REQUIRE(det.get("r_sole", c) && c.isActive && c.switchTime == time[2]);

    // the C ABI directly: six steps in one launch, its own triggers on the forces
    const blf::RobotModel m = bipedModel();
    blf::DeviceBuffer<int32_t> dParent, dFrameLink, dInts;
    blf::DeviceBuffer<double> dOrigin, dRot, dAxis, dMass, dCom, dInertia, dFramePose, dIn, dState, dOut;
    REQUIRE(dParent.upload(m.parent) && dFrameLink.upload(m.frameLink) && dOrigin.upload(m.jointOrigin)
            && dRot.upload(m.jointRotation) && dAxis.upload(m.jointAxis) && dMass.upload(m.linkMass)
            && dCom.upload(m.linkCom) && dInertia.upload(m.linkInertia) && dFramePose.upload(m.framePose));
    blf_fb_model dm{};
    dm.ndof = n;
    dm.nframes = K;
    dm.parent = dParent.data();
    dm.joint_origin = dOrigin.data();
    dm.joint_rot = dRot.data();
    dm.joint_axis = dAxis.data();
    dm.link_mass = dMass.data();
    dm.link_com = dCom.data();
    dm.link_inertia = dInertia.data();
    dm.frame_link = dFrameLink.data();
    dm.frame_pose = dFramePose.data();
    std::vector<double> in;   // time T | q T n | dq T n | force T K
    in.insert(in.end(), time.begin(), time.end());
    in.insert(in.end(), q.begin(), q.end());
    in.insert(in.end(), dq.begin(), dq.end());
    in.insert(in.end(), force.begin(), force.end());
    std::vector<double> state(2 * K + 12, 0.0);   // timers 2K | fixed_pose 12
    state[2 * K + 3] = state[2 * K + 7] = state[2 * K + 11] = 1.0;
    std::vector<int32_t> ints = {0, 1, /* trig_state */ 1, 0, /* fixed_frame */ 0, /* status */ -1};
    ints.resize(6 + T, -7);                       // fixed_out T
    REQUIRE(dIn.upload(in) && dState.upload(state) && dInts.upload(ints) && dOut.resize(T * 18));
    const double prm[4] = {10.0, 4.0, 0.0, 0.0};
    double* d = dIn.data();
    int32_t* i = dInts.data();
    REQUIRE(blf::report(blf_legged_odometry_advance(blf::threadHandle(), &dm, K, i, prm, 1, d, d + T, d + T + T * n,
                                                    d + T + 2 * T * n, T, i + 2, dState.data(), i + 4,
                                                    dState.data() + 2 * K, dOut.data(), dOut.data() + 3 * T,
                                                    dOut.data() + 12 * T, nullptr, i + 6, i + 5, 1, 0, nullptr),
                        "odometry_tests"));
    std::vector<double> out;
    REQUIRE(dOut.download(out) && dInts.download(ints) && dState.download(state));
    REQUIRE(ints[5] == BLF_IK_OK);
    for (int t = 0; t < T; ++t) REQUIRE(ints[6 + t] == fixed[t]);
    REQUIRE(same(out.data(), pos.data(), 3 * T));
    REQUIRE(same(out.data() + 3 * T, rot.data(), 9 * T));
    REQUIRE(same(out.data() + 12 * T, vel.data(), 6 * T));
    REQUIRE(same(state.data() + 2 * K, odo.getFixedFramePose().packed().data(), 12));

    // changeFixedFrame: the left sole again, at the pose the estimate gives it; the estimate does not move
    REQUIRE_FALSE(odo.changeFixedFrame("sole"));
    REQUIRE(odo.changeFixedFrame("l_sole"));
    REQUIRE(odo.getFixedFrameIdx() == 0);
    REQUIRE(odo.setContactStatus("l_sole", true, 0.07, 0.07));
    REQUIRE(odo.setContactStatus("r_sole", false, 0.07, 0.07));
    REQUIRE(odo.advance());
    REQUIRE(odo.getFixedFrameIdx() == 0);
    double worst = 0.0;
    for (int k = 0; k < 3; ++k) worst = std::max(worst, std::abs(odo.getOutput().basePose.position[k] - pos[3 * (T - 1) + k]));
    for (int k = 0; k < 9; ++k) worst = std::max(worst, std::abs(odo.getOutput().basePose.rotation[k] - rot[9 * (T - 1) + k]));
    REQUIRE(worst < 1e-12);
    // resetEstimator places the world at the fixed frame
    REQUIRE(odo.resetEstimator(blf::Transform::fromPlanar(1.0, 2.0, 0.5)));
    REQUIRE(odo.advance());
    REQUIRE(same(odo.getFixedFramePose().packed().data(), blf::Transform::fromPlanar(1.0, 2.0, 0.5).packed().data(), 12));
}

int main(int argc, char** argv)
{
    return runCases(argc, argv, {
        {"SchmittTriggerDetector state machine", false, testDetectorStateMachine},
        {"LeggedOdometry state machine", false, testOdometryStateMachine},
        {"Two-foot walk through the adapters", true, testWalkAgainstTheCAbi},
    });
}
