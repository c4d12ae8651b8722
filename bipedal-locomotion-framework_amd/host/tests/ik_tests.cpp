/**
 * @file ik_tests.cpp
 * Tests of the IK::SE3Task, IK::CoMTask, IK::JointTrackingTask and IK::QPInverseKinematics adapters,
 * with host_tests.cpp's conventions ("name ... ok", "N checks, 0 failed"; modes cpu / gpu / all):
 *   cpu: every path on which the adapters return false without touching a device (parameter
 *        handler errors, set points, addTask with priority 0 / a duplicate name / too many tasks /
 *        a wrong weight, finalize without a model, advance without a joint task or before finalize);
 *   gpu: on a 7-joint biped with the standing task set (two sole frames, CoM, posture), advance()
 *        equals blf_fb_ik_solve and is zero when every set point is met; a 20-step
 *        integration-based loop (advance, ForwardEuler<FloatingBaseSystemKinematics>, setRobotState)
 *        equals blf_fb_ik_integrate bit for bit.
 */
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include <hip/hip_runtime_api.h>

#include <BipedalLocomotion/IK/QPInverseKinematics.h>
#include <BipedalLocomotion/ParametersHandler/IParametersHandler.h>
#include <BipedalLocomotion/System/FloatingBaseSystemKinematics.h>
#include <BipedalLocomotion/System/ForwardEuler.h>

#include "test_harness.h"

using namespace BipedalLocomotion;
using namespace BipedalLocomotion::IK;
using namespace BipedalLocomotion::ParametersHandler;

static constexpr int kJoints = 7;

static std::shared_ptr<StdImplementation> se3Handler(int frame, double kpl = 4.0, double kpa = 3.0)
{
    auto h = std::make_shared<StdImplementation>();
    h->setParameter("frame_index", frame);
    h->setParameter("kp_linear", kpl);
    h->setParameter("kp_angular", kpa);
    return h;
}

static std::shared_ptr<SE3Task> se3Task(int frame)
{
    auto t = std::make_shared<SE3Task>();
    t->initialize(se3Handler(frame));
    return t;
}

static std::shared_ptr<CoMTask> comTask(double kp = 2.0)
{
    auto h = std::make_shared<StdImplementation>();
    h->setParameter("kp_linear", kp);
    auto t = std::make_shared<CoMTask>();
    t->initialize(h);
    return t;
}

static std::shared_ptr<JointTrackingTask> jointTask(int n = kJoints, double kp = 1.5)
{
    auto h = std::make_shared<StdImplementation>();
    h->setParameter("kp", std::vector<double>(n, kp));
    auto t = std::make_shared<JointTrackingTask>();
    t->initialize(h);
    return t;
}

static void testTaskParameters()
{
    {
        SE3Task task;
        std::weak_ptr<IParametersHandler> expired;
        {
            auto temporary = se3Handler(0);
            expired = temporary;
        }
        REQUIRE_FALSE(task.initialize(expired));
        REQUIRE_FALSE(task.isValid());
        REQUIRE(task.initialize(se3Handler(1)));
        REQUIRE(task.frameIndex() == 1 && task.kpLinear() == 4.0 && task.kpAngular() == 3.0);
        REQUIRE_FALSE(task.isValid());   // no set point yet
        REQUIRE(task.setSetPoint(blf::Transform::fromPlanar(0.1, 0.2, 0.3)));
        REQUIRE(task.isValid());
        blf::Transform bad;
        bad.position[1] = NAN;
        REQUIRE_FALSE(task.setSetPoint(bad));
        blf::Vector6 v{};
        v[4] = INFINITY;
        REQUIRE_FALSE(task.setSetPoint(blf::Transform::Identity(), v));
    }
    {
        auto h = std::make_shared<StdImplementation>();   // a frame by name
        h->setParameter("frame_name", "l_sole");
        h->setParameter("kp_linear", 1.0);
        h->setParameter("kp_angular", 0.0);
        SE3Task task;
        REQUIRE(task.initialize(h));
        REQUIRE(task.frameName() == "l_sole" && task.frameIndex() == -1);
    }
    for (const char* key : {"frame", "kp_linear", "kp_angular"})
    {
        auto h = std::make_shared<StdImplementation>();
        if (std::strcmp(key, "frame") != 0) h->setParameter("frame_index", 0);
        if (std::strcmp(key, "kp_linear") != 0) h->setParameter("kp_linear", 1.0);
        if (std::strcmp(key, "kp_angular") != 0) h->setParameter("kp_angular", 1.0);
        SE3Task task;
        REQUIRE_FALSE(task.initialize(h));
    }
    {
        SE3Task task;
        REQUIRE_FALSE(task.initialize(se3Handler(-1)));
        REQUIRE_FALSE(task.initialize(se3Handler(0, -1.0)));
        REQUIRE_FALSE(task.initialize(se3Handler(0, 1.0, NAN)));
    }
    {
        CoMTask task;
        REQUIRE_FALSE(task.initialize(std::make_shared<StdImplementation>()));
        auto h = std::make_shared<StdImplementation>();
        h->setParameter("kp_linear", -0.5);
        REQUIRE_FALSE(task.initialize(h));
        h->setParameter("kp_linear", 2.5);
        REQUIRE(task.initialize(h));
        REQUIRE(task.kpLinear() == 2.5);
        REQUIRE_FALSE(task.setSetPoint(blf::Vector3{{0.0, NAN, 0.0}}));
        REQUIRE(task.setSetPoint(blf::Vector3{{0.0, 0.1, 0.5}}, blf::Vector3{{0.1, 0.0, 0.0}}));
        REQUIRE(task.isValid() && task.velocity()[0] == 0.1);
    }
    {
        JointTrackingTask task;
        REQUIRE_FALSE(task.setSetPoint(blf::VectorXd(3, 0.0)));   // before initialize
        REQUIRE_FALSE(task.initialize(std::make_shared<StdImplementation>()));
        auto h = std::make_shared<StdImplementation>();
        h->setParameter("kp", std::vector<double>{1.0, -1.0, 1.0});
        REQUIRE_FALSE(task.initialize(h));
        h->setParameter("kp", std::vector<double>{1.0, 2.0, 3.0});
        REQUIRE(task.initialize(h));
        REQUIRE_FALSE(task.setSetPoint(blf::VectorXd(4, 0.0)));
        REQUIRE_FALSE(task.setSetPoint(blf::VectorXd(3, 0.0), blf::VectorXd(2, 0.0)));
        REQUIRE_FALSE(task.setSetPoint(blf::VectorXd{0.0, NAN, 0.0}));
        REQUIRE(task.setSetPoint(blf::VectorXd{0.1, 0.2, 0.3}));
        REQUIRE(task.isValid() && task.velocity().size() == 3 && task.velocity()[2] == 0.0);
    }
}

static void testTaskBookkeeping()
{
    const blf::VectorXd w6(6, 10.0), w3(3, 5.0), wn(kJoints, 0.1);
    {
        QPInverseKinematics ik;
        std::weak_ptr<IParametersHandler> expired;
        {
            auto temporary = std::make_shared<StdImplementation>();
            expired = temporary;
        }
        REQUIRE_FALSE(ik.initialize(expired));
        auto h = std::make_shared<StdImplementation>();
        REQUIRE(ik.initialize(h));   // base_damping is optional
        h->setParameter("base_damping", -1.0);
        REQUIRE_FALSE(ik.initialize(h));
        h->setParameter("base_damping", 1e-3);
        REQUIRE(ik.initialize(h));
    }
    {
        QPInverseKinematics ik;
        REQUIRE_FALSE(ik.addTask(se3Task(0), "hard", 0, w6));          // priority 0: hard constraints
        REQUIRE_FALSE(ik.addTask(se3Task(0), "low", 2, w6));
        REQUIRE_FALSE(ik.addTask(nullptr, "null", 1, w6));
        REQUIRE_FALSE(ik.addTask(se3Task(0), "short", 1, w3));         // one weight per row
        REQUIRE_FALSE(ik.addTask(se3Task(0), "none", 1));
        REQUIRE_FALSE(ik.addTask(se3Task(0), "negative", 1, blf::VectorXd{1, 1, 1, -1, 1, 1}));
        REQUIRE_FALSE(ik.addTask(se3Task(0), "nan", 1, blf::VectorXd{1, 1, NAN, 1, 1, 1}));
        REQUIRE(ik.getTaskNames().empty());
        REQUIRE(ik.addTask(se3Task(0), "left", 1, w6));
        REQUIRE_FALSE(ik.addTask(se3Task(1), "left", 1, w6));          // duplicate name
        REQUIRE(ik.addTask(se3Task(1), "right", 1, blf::VectorXd{0, 0, 0, 1, 1, 1}));   // SO3-only
        REQUIRE(ik.addTask(se3Task(0), "third", 1, w6));
        REQUIRE(ik.addTask(se3Task(1), "fourth", 1, w6));
        REQUIRE_FALSE(ik.addTask(se3Task(1), "fifth", 1, w6));         // BLF_IK_MAX_SE3_TASKS
        REQUIRE(ik.addTask(comTask(), "com", 1, w3));
        REQUIRE_FALSE(ik.addTask(comTask(), "com2", 1, w3));
        REQUIRE_FALSE(ik.addTask(comTask(), "com3", 1, w6));
        REQUIRE_FALSE(ik.advance());                                    // no joint tracking task
        REQUIRE_FALSE(ik.isValid());
        REQUIRE_FALSE(ik.addTask(jointTask(), "zero", 1, blf::VectorXd(kJoints, 0.0)));   // must be > 0
        REQUIRE(ik.addTask(jointTask(), "posture", 1, wn));
        REQUIRE_FALSE(ik.addTask(jointTask(), "posture2", 1, wn));
        REQUIRE(ik.getTaskNames().size() == 6);
        REQUIRE_FALSE(ik.advance());                                    // before finalize
        REQUIRE_FALSE(ik.finalize());                                   // no robot model
        REQUIRE_FALSE(ik.setRobotState(blf::Vector3{}, blf::Transform::Identity().rotation, blf::VectorXd(kJoints)));
        blf::RobotModel corrupted;
        corrupted.ndof = 2;
        corrupted.parent = {0};
        REQUIRE_FALSE(ik.setRobotModel(corrupted));
        REQUIRE_FALSE(ik.isValid());
    }
}

// ---- device cases -------------------------------------------------------------------------------
// pelvis, two legs of three pitch / roll joints each, one torso joint; sole frames on the feet
static blf::RobotModel bipedModel()
{
    blf::RobotModel m;
    m.ndof = kJoints;
    m.parent = {0, 1, 2, 0, 4, 5, 0};
    m.jointOrigin = {0.0, 0.08, -0.05, 0.0, 0.0, -0.25, 0.0, 0.0, -0.25,
                     0.0, -0.08, -0.05, 0.0, 0.0, -0.25, 0.0, 0.0, -0.25, 0.0, 0.0, 0.1};
    for (int j = 0; j < kJoints; ++j) m.jointRotation.insert(m.jointRotation.end(), {1, 0, 0, 0, 1, 0, 0, 0, 1});
    m.jointAxis = {0, 1, 0, 0, 1, 0, 1, 0, 0, 0, 1, 0, 0, 1, 0, 1, 0, 0, 0, 0, 1};
    m.linkMass = {6.0, 2.0, 1.5, 0.8, 2.0, 1.5, 0.8, 5.0};
    m.linkCom = {0.0, 0.0, 0.02, 0.0, 0.0, -0.12, 0.0, 0.0, -0.12, 0.03, 0.0, -0.02,
                 0.0, 0.0, -0.12, 0.0, 0.0, -0.12, 0.03, 0.0, -0.02, 0.0, 0.0, 0.15};
    for (double mass : m.linkMass)
        m.linkInertia.insert(m.linkInertia.end(), {0.01 * mass, 0, 0, 0, 0.012 * mass, 0, 0, 0, 0.008 * mass});
    m.frameLink = {3, 6};
    m.framePose = {0.02, 0.0, -0.04, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0.02, 0.0, -0.04, 1, 0, 0, 0, 1, 0, 0, 0, 1};
    return m;
}

static const blf::Vector3 kBase0{{0.01, -0.02, 0.6}};
static blf::VectorXd joints0()
{
    return blf::VectorXd{-0.3, 0.6, 0.05, -0.25, 0.5, -0.04, 0.1};
}

struct Standing
{
    QPInverseKinematics ik;
    std::shared_ptr<SE3Task> left, right;
    std::shared_ptr<CoMTask> com;
    std::shared_ptr<JointTrackingTask> posture;
};

// the standing set by frame names; the set points are the caller's
static bool makeStanding(Standing& s)
{
    auto h = std::make_shared<StdImplementation>();
    h->setParameter("base_damping", 1e-3);
    bool ok = s.ik.initialize(h);
    ok = ok && s.ik.setRobotModel(bipedModel(), {"l_sole", "r_sole"});
    auto named = [](const char* name) {
        auto hh = std::make_shared<StdImplementation>();
        hh->setParameter("frame_name", name);
        hh->setParameter("kp_linear", 4.0);
        hh->setParameter("kp_angular", 3.0);
        auto t = std::make_shared<SE3Task>();
        t->initialize(hh);
        return t;
    };
    s.left = named("l_sole");
    s.right = named("r_sole");
    s.com = comTask();
    s.posture = jointTask();
    ok = ok && s.ik.addTask(s.left, "left_foot", 1, blf::VectorXd(6, 20.0));
    ok = ok && s.ik.addTask(s.right, "right_foot", 1, blf::VectorXd(6, 20.0));
    ok = ok && s.ik.addTask(s.com, "com", 1, blf::VectorXd(3, 10.0));
    ok = ok && s.ik.addTask(s.posture, "posture", 1, blf::VectorXd(kJoints, 0.1));
    return ok && s.ik.finalize();
}

static void setPoints(Standing& s)
{
    s.left->setSetPoint(blf::Transform::fromPlanar(0.03, 0.09, 0.05), blf::Vector6{{0.01, 0, 0, 0, 0, 0.02}});
    s.right->setSetPoint(blf::Transform::fromPlanar(0.02, -0.09, -0.04));
    s.com->setSetPoint(blf::Vector3{{0.02, 0.0, 0.45}}, blf::Vector3{{0.0, 0.01, 0.0}});
    s.posture->setSetPoint(blf::VectorXd{-0.2, 0.4, 0.0, -0.2, 0.4, 0.0, 0.0});
}

static void testAdvanceOnDevice()
{
    {
        QPInverseKinematics ik;   // an unknown frame name is refused at finalize
        REQUIRE(ik.setRobotModel(bipedModel(), {"l_sole", "r_sole"}));
        auto hh = std::make_shared<StdImplementation>();
        hh->setParameter("frame_name", "head");
        hh->setParameter("kp_linear", 1.0);
        hh->setParameter("kp_angular", 1.0);
        auto t = std::make_shared<SE3Task>();
        REQUIRE(t->initialize(hh));
        REQUIRE(ik.addTask(t, "head", 1, blf::VectorXd(6, 1.0)));
        REQUIRE_FALSE(ik.finalize());
        REQUIRE_FALSE(ik.setRobotModel(bipedModel(), {"only_one"}));
    }
    Standing s;
    REQUIRE(makeStanding(s));
    REQUIRE_FALSE(s.ik.advance());   // no robot state, no set points
    const blf::Matrix3 R0 = blf::Transform::fromPlanar(0, 0, 0.1).rotation;
    REQUIRE_FALSE(s.ik.setRobotState(kBase0, R0, blf::VectorXd(3, 0.0)));
    REQUIRE(s.ik.setRobotState(kBase0, R0, joints0()));
    REQUIRE_FALSE(s.ik.advance());   // tasks without set points
    setPoints(s);
    REQUIRE(s.ik.advance());
    REQUIRE(s.ik.isValid());
    const IntegrationBasedIKState got = s.ik.get();
    REQUIRE(got.jointVelocity.size() == kJoints);
    // the same solve through the C ABI, on the adapter's device arrays
    blf::DeviceBuffer<double> out(6 + kJoints);
    REQUIRE(blf_fb_ik_solve(blf::threadHandle(), &s.ik.deviceModel(), &s.ik.deviceState(), &s.ik.deviceTasks(),
                            1, out.data(), nullptr, nullptr) == BLF_OK);
    std::vector<double> nu;
    REQUIRE(out.download(nu));
    REQUIRE(std::memcmp(nu.data(), got.baseVelocity.data(), 6 * sizeof(double)) == 0);
    REQUIRE(std::memcmp(nu.data() + 6, got.jointVelocity.data(), kJoints * sizeof(double)) == 0);
    double norm = 0.0;
    for (double v : nu) norm += v * v;
    REQUIRE(std::isfinite(norm) && norm > 1e-6);
    // every set point met (the frames' and the CoM's own values, from blf_fb_frame_state / blf_fb_dcm)
    // and no feed-forward: nu = 0
    blf::DeviceBuffer<int32_t> frames;
    REQUIRE(frames.upload(std::vector<int32_t>{0, 1}));
    blf::DeviceBuffer<double> poses(24), com(6);
    REQUIRE(blf_fb_frame_state(blf::threadHandle(), &s.ik.deviceModel(), &s.ik.deviceState(), 2, frames.data(), 1,
                               poses.data(), nullptr, nullptr) == BLF_OK);
    REQUIRE(blf_fb_dcm(blf::threadHandle(), &s.ik.deviceModel(), &s.ik.deviceState(), nullptr, 0, 1, com.data(),
                       nullptr, nullptr) == BLF_OK);
    std::vector<double> hp, hc;
    REQUIRE(poses.download(hp) && com.download(hc));
    blf::Transform tl, tr;
    std::copy(hp.begin(), hp.begin() + 3, tl.position.begin());
    std::copy(hp.begin() + 3, hp.begin() + 12, tl.rotation.begin());
    std::copy(hp.begin() + 12, hp.begin() + 15, tr.position.begin());
    std::copy(hp.begin() + 15, hp.begin() + 24, tr.rotation.begin());
    REQUIRE(s.left->setSetPoint(tl) && s.right->setSetPoint(tr));
    REQUIRE(s.com->setSetPoint(blf::Vector3{{hc[0], hc[1], hc[2]}}));
    REQUIRE(s.posture->setSetPoint(joints0()));
    REQUIRE(s.ik.advance());
    for (int i = 0; i < 6; ++i) REQUIRE(std::abs(s.ik.get().baseVelocity[i]) < 1e-12);
    for (int i = 0; i < kJoints; ++i) REQUIRE(std::abs(s.ik.get().jointVelocity[i]) < 1e-12);
    // a NaN state: the device reports the robot, advance() returns false
    blf::VectorXd q = joints0();
    q[2] = NAN;
    REQUIRE(s.ik.setRobotState(kBase0, R0, q));
    REQUIRE_FALSE(s.ik.advance());
    REQUIRE_FALSE(s.ik.isValid());
}

static void testIntegrationLoopOnDevice()
{
    constexpr int steps = 20;
    constexpr double dT = 0.01;
    Standing s;
    REQUIRE(makeStanding(s));
    setPoints(s);
    const blf::Matrix3 R0 = blf::Transform::fromPlanar(0, 0, 0.1).rotation;
    REQUIRE(s.ik.setRobotState(kBase0, R0, joints0()));
    REQUIRE(s.ik.advance());
    // the fused loop, in place on the adapter's device arrays (the next advance() uploads them anew)
    const blf_fb_state st = s.ik.deviceState();
    blf::DeviceBuffer<double> nuBuf(6 + kJoints);
    blf::DeviceBuffer<int32_t> statusBuf(1);
    REQUIRE(blf_fb_ik_integrate(blf::threadHandle(), &s.ik.deviceModel(), &st, &s.ik.deviceTasks(), 1, steps, dT,
                                nuBuf.data(), statusBuf.data(), nullptr) == BLF_OK);
    std::vector<double> fp(3), fR(9), fq(kJoints), fnu;
    std::vector<int32_t> fstatus;
    REQUIRE(hipMemcpy(fp.data(), st.base_pos, 3 * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess);
    REQUIRE(hipMemcpy(fR.data(), st.base_rot, 9 * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess);
    REQUIRE(hipMemcpy(fq.data(), st.joint_pos, kJoints * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess);
    REQUIRE(nuBuf.download(fnu) && statusBuf.download(fstatus));
    REQUIRE(fstatus[0] == BLF_IK_OK);

    // the same loop through the adapters: advance, one Euler step of dT, the new state back
    auto system = std::make_shared<System::FloatingBaseSystemKinematics>();
    auto handler = std::make_shared<StdImplementation>();
    handler->setParameter("rho", 0.01);
    REQUIRE(system->initalize(handler));
    System::ForwardEuler<System::FloatingBaseSystemKinematics> integrator(dT);
    REQUIRE(integrator.setDynamicalSystem(system));
    REQUIRE(system->setState({kBase0, R0, joints0()}));
    for (int k = 0; k < steps; ++k)
    {
        const auto& [p, R, q] = integrator.getSolution();
        REQUIRE(s.ik.setRobotState(p, R, q));
        REQUIRE(s.ik.advance());
        REQUIRE(system->setControlInput({s.ik.get().baseVelocity, s.ik.get().jointVelocity}));
        REQUIRE(integrator.integrate(0.0, dT));
    }
    const auto& [p, R, q] = integrator.getSolution();
    REQUIRE(std::memcmp(p.data(), fp.data(), 3 * sizeof(double)) == 0);
    REQUIRE(std::memcmp(R.data(), fR.data(), 9 * sizeof(double)) == 0);
    REQUIRE(std::memcmp(q.data(), fq.data(), kJoints * sizeof(double)) == 0);
    REQUIRE(std::memcmp(s.ik.get().baseVelocity.data(), fnu.data(), 6 * sizeof(double)) == 0);
    REQUIRE(std::memcmp(s.ik.get().jointVelocity.data(), fnu.data() + 6, kJoints * sizeof(double)) == 0);
    // the loop did move the robot towards the set points
    REQUIRE(std::abs(fq[1] - joints0()[1]) > 1e-3);
}

int main(int argc, char** argv)
{
    return runCases(argc, argv, {
        {"IK tasks parameter handler", false, testTaskParameters},
        {"QPInverseKinematics task bookkeeping", false, testTaskBookkeeping},
        {"QPInverseKinematics on the device", true, testAdvanceOnDevice},
        {"IntegrationBasedIK loop on the device", true, testIntegrationLoopOnDevice},
    });
}
