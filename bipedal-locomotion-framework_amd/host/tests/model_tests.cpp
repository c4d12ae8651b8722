/**
 * @file model_tests.cpp
 * Tests of blf/robot_model.h, what the adapters over a blf_fb_model share, with host_tests.cpp's
 * conventions ("name ... ok", "N checks, 0 failed"; modes cpu / gpu / all):
 *   cpu: prepareRobotModel's defects in the order the header fixes, each refused by the three adapters
 *        with the one text (a "model_tests row" line on stderr precedes every row's three refusals and
 *        carries the text they have to contain: tests/test_host_model.py reads them); the fixed-joint
 *        models FloatingBaseDynamicalSystem used to accept unmerged; accepted models; the state layout;
 *   gpu: blf_fb_frame_state through DeviceRobotModel::view against a hand-uploaded blf_fb_model, bit
 *        for bit, also after set() has replaced a larger model that had joint types.
 */
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include <BipedalLocomotion/FloatingBaseEstimators/LeggedOdometry.h>
#include <BipedalLocomotion/IK/QPInverseKinematics.h>
#include <BipedalLocomotion/ParametersHandler/IParametersHandler.h>
#include <BipedalLocomotion/System/FloatingBaseSystemDynamics.h>
#include <blf/robot_model.h>

#include "ik_fixtures.h"
#include "model_fixtures.h"
#include "test_harness.h"

using namespace BipedalLocomotion;
using blf::ModelDefect;

// whether each adapter refuses the model (every frame is named "0", "1", ... for the odometry)
static bool dynamicsRefuses(const blf::RobotModel& m)
{
    System::FloatingBaseDynamicalSystem system;
    return !system.setRobotModel(m);
}
static bool ikRefuses(const blf::RobotModel& m)
{
    IK::QPInverseKinematics ik;
    return !ik.setRobotModel(m);
}
static bool odometryRefuses(const blf::RobotModel& m)
{
    auto handler = std::make_shared<ParametersHandler::StdImplementation>();
    handler->setParameter("initial_fixed_frame", std::string("0"));
    Estimators::LeggedOdometry odometry;
    return odometry.initialize(handler) && !odometry.setRobotModel(m);
}

static void oneFrameOn(blf::RobotModel& m, int32_t link)
{
    m.frameLink = {link};
    m.framePose.resize(12);
}

struct Row
{
    const char* name;
    std::function<void(blf::RobotModel&)> mutate;
    ModelDefect plain, masked;   // expected without and with a fixedJoint mask
};

static void testDefectTable()
{
    const ModelDefect C = ModelDefect::Corrupted, T = ModelDefect::NotTopological,
                      F = ModelDefect::FrameOnUnknownLink, U = ModelDefect::UnknownJointType;
    auto badOrder = [](blf::RobotModel& m) { m.parent[1] = 2; };
    auto badType = [](blf::RobotModel& m) {
        m.jointType.assign(m.parent.size(), BLF_JOINT_REVOLUTE);
        m.jointType[0] = 5;
    };
    auto lowerOnly = [](blf::RobotModel& m) { m.jointLower.assign(m.parent.size(), -1.0); };
    const std::vector<Row> rows = {
        {"a popped jointAxis", [](blf::RobotModel& m) { m.jointAxis.pop_back(); }, C, C},
        {"ndof 0", [](blf::RobotModel& m) { m.ndof = 0; }, C, C},
        {"ndof 49", [](blf::RobotModel& m) { m.ndof = 49; }, C, C},
        {"jointType of n - 1", [](blf::RobotModel& m) { m.jointType.assign(m.parent.size() - 1, BLF_JOINT_REVOLUTE); }, C, C},
        {"jointLower without jointUpper", lowerOnly, C, C},
        {"jointVelocityLimit of 2", [](blf::RobotModel& m) { m.jointVelocityLimit.assign(2, 1.0); }, C, C},
        {"parent[1] = 2", badOrder, T, T},
        {"a frame on link n + 1", [](blf::RobotModel& m) { oneFrameOn(m, m.ndof + 1); }, F, F},
        {"a frame on link -1", [](blf::RobotModel& m) { oneFrameOn(m, -1); }, F, F},
        {"joint type 5", badType, U, U},
        // two defects: the earlier check reports
        {"a popped jointAxis and parent[1] = 2", [&](blf::RobotModel& m) { m.jointAxis.pop_back(); badOrder(m); }, C, C},
        {"parent[1] = 2 and a frame on link -1", [&](blf::RobotModel& m) { badOrder(m); oneFrameOn(m, -1); }, T, T},
        {"a frame on link -1 and joint type 5", [&](blf::RobotModel& m) { oneFrameOn(m, -1); badType(m); }, F, F},
        // the limits' lengths are compared after the merge (check 5), the order before it (check 2)
        {"jointLower without jointUpper and parent[1] = 2", [&](blf::RobotModel& m) { lowerOnly(m); badOrder(m); }, C, T},
    };
    for (const char* base : {"chain", "biped"})
        for (const bool mask : {false, true})
            for (const Row& row : rows)
            {
                blf::RobotModel m = std::strcmp(base, "chain") == 0 ? chainModel() : bipedModel();
                if (mask)   // valid: the last joint fixed
                {
                    m.fixedJoint.assign(m.parent.size(), 0);
                    m.fixedJoint.back() = 1;
                }
                row.mutate(m);
                const ModelDefect expected = mask ? row.masked : row.plain;
                blf::RobotModel reduced;
                REQUIRE(blf::prepareRobotModel(m, reduced) == expected);
                std::fprintf(stderr, "model_tests row %s, %s%s: %s\n", base, row.name, mask ? ", masked" : "",
                             blf::describe(expected));
                REQUIRE(dynamicsRefuses(m));
                REQUIRE(ikRefuses(m));
                REQUIRE(odometryRefuses(m));
            }
    std::fprintf(stderr, "model_tests end of rows\n");
    REQUIRE(std::strcmp(blf::describe(ModelDefect::None), "") == 0);
}

static void testFixedJointHole()
{
    blf::RobotModel reduced;
    blf::RobotModel m = chainModel();
    m.fixedJoint = {0, 1, 0};
    m.frameLink = {9};
    REQUIRE(blf::reduceFixedJoints(m).fixedJoint.size() == 3);   // not merged
    REQUIRE(blf::prepareRobotModel(m, reduced) == ModelDefect::FrameOnUnknownLink);
    REQUIRE(dynamicsRefuses(m));
    m = chainModel();
    m.fixedJoint = {0, 1, 0};
    m.jointLower.assign(2, -1.0);
    REQUIRE(blf::reduceFixedJoints(m).fixedJoint.size() == 3);
    REQUIRE(blf::prepareRobotModel(m, reduced) == ModelDefect::Corrupted);
    REQUIRE(dynamicsRefuses(m));
}

static bool sameModel(const blf::RobotModel& a, const blf::RobotModel& b)
{
    return a.ndof == b.ndof && a.parent == b.parent && a.jointOrigin == b.jointOrigin
           && a.jointRotation == b.jointRotation && a.jointAxis == b.jointAxis && a.linkMass == b.linkMass
           && a.linkCom == b.linkCom && a.linkInertia == b.linkInertia && a.frameLink == b.frameLink
           && a.framePose == b.framePose && a.fixedJoint == b.fixedJoint && a.jointType == b.jointType
           && a.jointLower == b.jointLower && a.jointUpper == b.jointUpper
           && a.jointVelocityLimit == b.jointVelocityLimit;
}

static void testAcceptedModels()
{
    blf::RobotModel fixedChain = chainModel();
    fixedChain.fixedJoint = {0, 1, 1};
    fixedChain.jointType = {BLF_JOINT_PRISMATIC, BLF_JOINT_REVOLUTE, BLF_JOINT_REVOLUTE};
    fixedChain.jointLower = {-1.0, -2.0, -3.0};
    fixedChain.jointUpper = {1.0, 2.0, 3.0};
    fixedChain.jointVelocityLimit = {4.0, 5.0, 6.0};
    for (const blf::RobotModel& full : {chainModel(), bipedModel(), fixedChain})
    {
        blf::RobotModel reduced;
        REQUIRE(blf::prepareRobotModel(full, reduced) == ModelDefect::None);
        REQUIRE(sameModel(reduced, blf::reduceFixedJoints(full)));
        REQUIRE(reduced.fixedJoint.empty());
    }
    blf::RobotModel reduced;
    REQUIRE(blf::prepareRobotModel(fixedChain, reduced) == ModelDefect::None);
    REQUIRE(reduced.ndof == 1 && reduced.jointType == std::vector<int32_t>{BLF_JOINT_PRISMATIC});
    REQUIRE(reduced.jointUpper == std::vector<double>{1.0} && reduced.jointVelocityLimit == std::vector<double>{4.0});
}

static void testStateLayout()
{
    for (const std::size_t n : {std::size_t(1), std::size_t(13)})
    {
        REQUIRE(blf::fbStateSize(n) == 18 + 2 * n);
        std::vector<double> s(blf::fbStateSize(n), -1.0);
        const blf_fb_state at = blf::fbStateAt(s.data(), n);
        REQUIRE(at.base_vel - s.data() == 0 && at.joint_vel - s.data() == 6);
        REQUIRE(at.base_pos - s.data() == static_cast<std::ptrdiff_t>(6 + n));
        REQUIRE(at.base_rot - s.data() == static_cast<std::ptrdiff_t>(9 + n));
        REQUIRE(at.joint_pos - s.data() == static_cast<std::ptrdiff_t>(18 + n));
        blf::Vector6 bv, bv2{};
        blf::Vector3 bp, bp2{};
        blf::Matrix3 bR, bR2{};
        blf::VectorXd jv(n), jp(n), jv2, jp2(3, 0.0);
        double next = 1.0;   // every entry its own value, in the layout's order
        for (double& x : bv) x = next++;
        for (std::size_t i = 0; i < n; ++i) jv[i] = next++;
        for (double& x : bp) x = next++;
        for (double& x : bR) x = next++;
        for (std::size_t i = 0; i < n; ++i) jp[i] = next++;
        blf::fbStatePack(bv, jv, bp, bR, jp, s.data());
        bool counted = true;
        for (std::size_t i = 0; i < s.size(); ++i) counted = counted && s[i] == static_cast<double>(i + 1);
        REQUIRE(counted);
        blf::fbStateUnpack(s.data(), n, bv2, jv2, bp2, bR2, jp2);
        REQUIRE(bv2 == bv && bp2 == bp && bR2 == bR && jv2.size() == n && jp2.size() == n);
        bool same = true;
        for (std::size_t i = 0; i < n && jv2.size() == n && jp2.size() == n; ++i)
            same = same && jv2[i] == jv[i] && jp2[i] == jp[i];
        REQUIRE(same);
    }
}

// pose 12 F | twist 6 F of every frame of the model at one fixed, non-trivial state
static std::vector<double> frameStates(const blf_fb_model& model)
{
    const std::size_t n = static_cast<std::size_t>(model.ndof), F = static_cast<std::size_t>(model.nframes);
    blf::Vector6 bv{{0.1, -0.2, 0.3, 0.4, -0.5, 0.6}};
    blf::Vector3 bp{{0.3, -0.1, 0.9}};
    const double c = std::cos(0.4), s = std::sin(0.4);
    blf::Matrix3 bR{{c, -s, 0.0, s, c, 0.0, 0.0, 0.0, 1.0}};
    blf::VectorXd jv(n), jp(n);
    for (std::size_t j = 0; j < n; ++j)
    {
        jv[j] = 0.2 * std::cos(0.4 * j + 0.1);
        jp[j] = 0.3 * std::sin(0.7 * j + 0.2);
    }
    std::vector<double> host(blf::fbStateSize(n)), out(18 * F, 0.0);
    blf::fbStatePack(bv, jv, bp, bR, jp, host.data());
    std::vector<int32_t> frames(F);
    for (std::size_t f = 0; f < F; ++f) frames[f] = static_cast<int32_t>(f);
    blf::DeviceBuffer<double> dState, dOut;
    blf::DeviceBuffer<int32_t> dFrames;
    REQUIRE(dState.upload(host) && dFrames.upload(frames) && dOut.upload(out));
    const blf_fb_state state = blf::fbStateAt(dState.data(), n);
    REQUIRE(blf::report(blf_fb_frame_state(blf::threadHandle(), &model, &state, static_cast<int32_t>(F), dFrames.data(),
                                           1, dOut.data(), dOut.data() + 12 * F, nullptr),
                        "model_tests"));
    REQUIRE(dOut.download(out));
    return out;
}

// the model uploaded array by array, as a caller of the C ABI does without the adapters
struct HandUpload
{
    blf::DeviceBuffer<int32_t> parent, frameLink, jointType;
    blf::DeviceBuffer<double> origin, rot, axis, mass, com, inertia, framePose;
    blf_fb_model model{};

    explicit HandUpload(const blf::RobotModel& m)
    {
        REQUIRE(parent.upload(m.parent) && frameLink.upload(m.frameLink) && origin.upload(m.jointOrigin)
                && rot.upload(m.jointRotation) && axis.upload(m.jointAxis) && mass.upload(m.linkMass)
                && com.upload(m.linkCom) && inertia.upload(m.linkInertia) && framePose.upload(m.framePose));
        model.ndof = m.ndof;
        model.nframes = static_cast<int32_t>(m.frameLink.size());
        model.parent = parent.data();
        model.joint_origin = origin.data();
        model.joint_rot = rot.data();
        model.joint_axis = axis.data();
        model.link_mass = mass.data();
        model.link_com = com.data();
        model.link_inertia = inertia.data();
        model.frame_link = frameLink.data();
        model.frame_pose = framePose.data();
        model.gravity[2] = -9.81;
        model.rho = 0.01;
        if (!m.jointType.empty())
        {
            REQUIRE(jointType.upload(m.jointType));
            model.joint_type = jointType.data();
        }
    }
};

static const double kGravity[3] = {0.0, 0.0, -9.81};

static void requireSameFrames(const blf::DeviceRobotModel& device, const blf::RobotModel& m)
{
    REQUIRE(device.ok() && sameModel(device.host(), m));
    const blf_fb_model view = device.view(kGravity, 0.01);
    REQUIRE(view.ndof == m.ndof && view.nframes == static_cast<int32_t>(m.frameLink.size()));
    REQUIRE((view.joint_type == nullptr) == m.jointType.empty());
    REQUIRE(view.gravity[0] == 0.0 && view.gravity[1] == 0.0 && view.gravity[2] == -9.81 && view.rho == 0.01);
    const HandUpload hand(m);
    const std::vector<double> a = frameStates(view), b = frameStates(hand.model);
    REQUIRE(a.size() == 18 * m.frameLink.size() && a.size() == b.size());
    REQUIRE(a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0);
    bool finite = true;
    for (const double x : a) finite = finite && std::isfinite(x);
    REQUIRE(finite);
}

static void testDeviceModel()
{
    REQUIRE(blf::threadHandle() != nullptr);
    blf::RobotModel prismatic = chainModel();
    prismatic.jointType = {BLF_JOINT_REVOLUTE, BLF_JOINT_PRISMATIC, BLF_JOINT_REVOLUTE};
    for (const blf::RobotModel& m : {chainModel(), prismatic, bipedModel()})
    {
        blf::DeviceRobotModel device;
        REQUIRE(!device.ok());
        REQUIRE(device.set(m));
        requireSameFrames(device, m);
    }
    // one object: joint types, then a larger model without them, then every buffer shrinks
    blf::DeviceRobotModel device;
    for (const blf::RobotModel& m : {prismatic, bipedModel(), chainModel()})
    {
        REQUIRE(device.set(m));
        requireSameFrames(device, m);
    }
    blf::DeviceRobotModel moved(std::move(device));
    REQUIRE(moved.ok() && !device.ok());
    requireSameFrames(moved, chainModel());
}

int main(int argc, char** argv)
{
    return runCases(argc, argv, {
        {"defect table", false, testDefectTable},
        {"the fixed-joint hole", false, testFixedJointHole},
        {"accepted models", false, testAcceptedModels},
        {"state layout", false, testStateLayout},
        {"device model", true, testDeviceModel},
    });
}
