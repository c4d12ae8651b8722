/**
 * @file ik_priority_tests.cpp
 * Tests of IK::QPInverseKinematics::setTaskPriority, the adapter's form of a contact flag, with
 * ik_tests.cpp's conventions ("name ... ok", "N checks, 0 failed"; modes cpu / gpu / all):
 *   cpu: a weighted SE3 or CoM task switches to hard and back and hardRows() follows; refused for an
 *        unknown name, a priority above 1, the joint tracking and joint limits tasks, a task added at
 *        priority 0 and a task with a zero weight, the task keeping its priority;
 *   gpu: on a 13-joint biped whose feet were added weighted, advance() after switching one foot, then
 *        both, to priority 0 equals blf_fb_ik_solve_hard with the corresponding mask on the adapter's
 *        device arrays (the rows enter H with the weights the task was added with), and after switching
 *        back equals blf_fb_ik_solve.
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

#include "ik_fixtures.h"
#include "test_harness.h"

using namespace BipedalLocomotion;
using namespace BipedalLocomotion::IK;
using namespace BipedalLocomotion::ParametersHandler;

static std::shared_ptr<JointLimitsTask> limitsTask()
{
    auto h = std::make_shared<StdImplementation>();
    h->setParameter("klim", std::vector<double>(kJoints, 0.5));
    h->setParameter("sampling_time", 0.01);
    h->setParameter("use_model_limits", false);
    h->setParameter("lower_limits", std::vector<double>(kJoints, -1.0));
    h->setParameter("upper_limits", std::vector<double>(kJoints, 1.0));
    auto t = std::make_shared<JointLimitsTask>();
    t->initialize(h);
    return t;
}

static void testPriorityBookkeeping()
{
    QPInverseKinematics ik;
    REQUIRE(ik.initialize(std::make_shared<StdImplementation>()));
    blf::VectorXd partial(6, 10.0);
    partial[4] = 0.0;
    REQUIRE(ik.addTask(se3Task(0), "left_foot", 1, blf::VectorXd(6, 10.0)));
    REQUIRE(ik.addTask(se3Task(1), "right_foot", 1, blf::VectorXd(6, 7.0)));
    REQUIRE(ik.addTask(se3Task(1), "hand", 1, partial));
    REQUIRE(ik.addTask(se3Task(0), "pinned", 0));
    REQUIRE(ik.addTask(comTask(), "com", 1, blf::VectorXd(3, 5.0)));
    REQUIRE(ik.addTask(jointTask(), "posture", 1, blf::VectorXd(kJoints, 0.1)));
    REQUIRE(ik.addTask(limitsTask(), "limits", 0));
    const uint32_t pinned = 0x3fu << 18;
    REQUIRE(ik.hardRows() == pinned);
    // a stance foot, then both, then the CoM
    REQUIRE(ik.setTaskPriority("left_foot", 0));
    REQUIRE(ik.hardRows() == (pinned | 0x3fu));
    REQUIRE(ik.setTaskPriority("left_foot", 0));   // again: no change
    REQUIRE(ik.hardRows() == (pinned | 0x3fu));
    REQUIRE(ik.setTaskPriority("right_foot", 0));
    REQUIRE(ik.hardRows() == (pinned | 0xfffu));
    REQUIRE(ik.setTaskPriority("com", 0));
    REQUIRE(ik.hardRows() == (pinned | 0xfffu | (0x7u << 24)));
    // lift-off
    REQUIRE(ik.setTaskPriority("left_foot", 1));
    REQUIRE(ik.hardRows() == (pinned | (0x3fu << 6) | (0x7u << 24)));
    REQUIRE(ik.setTaskPriority("com", 1));
    REQUIRE(ik.setTaskPriority("right_foot", 1));
    REQUIRE(ik.hardRows() == pinned);
    // refusals: the task keeps its priority
    REQUIRE_FALSE(ik.setTaskPriority("nobody", 0));
    REQUIRE_FALSE(ik.setTaskPriority("left_foot", 2));
    REQUIRE_FALSE(ik.setTaskPriority("posture", 0));
    REQUIRE_FALSE(ik.setTaskPriority("posture", 1));
    REQUIRE_FALSE(ik.setTaskPriority("limits", 1));
    REQUIRE_FALSE(ik.setTaskPriority("pinned", 1));   // added at priority 0: no weights of its own
    REQUIRE_FALSE(ik.setTaskPriority("pinned", 0));
    REQUIRE_FALSE(ik.setTaskPriority("hand", 0));     // a zero weight
    REQUIRE(ik.hardRows() == pinned);
    REQUIRE(ik.getTaskNames().size() == 7);
}

struct Biped
{
    QPInverseKinematics ik;
    std::shared_ptr<SE3Task> left, right;
    std::shared_ptr<CoMTask> com;
    std::shared_ptr<JointTrackingTask> posture;
};

// The standing set with every task weighted: the feet with different weights, so that a hard foot's
// rows can be told to enter H with its own.
static bool makeBiped(Biped& s)
{
    bool ok = s.ik.initialize(std::make_shared<StdImplementation>());
    ok = ok && s.ik.setRobotModel(bipedModel(), {"l_sole", "r_sole"});
    s.left = se3Task(0);
    s.right = se3Task(1);
    s.com = comTask();
    s.posture = jointTask();
    ok = ok && s.ik.addTask(s.left, "left_foot", 1, blf::VectorXd(6, 12.0));
    ok = ok && s.ik.addTask(s.right, "right_foot", 1, blf::VectorXd(6, 9.0));
    ok = ok && s.ik.addTask(s.com, "com", 1, blf::VectorXd(3, 10.0));
    ok = ok && s.ik.addTask(s.posture, "posture", 1, blf::VectorXd(kJoints, 0.1));
    ok = ok && s.ik.finalize();
    s.left->setSetPoint(blf::Transform::fromPlanar(0.03, 0.09, 0.05), blf::Vector6{{0.01, 0, 0, 0, 0, 0.02}});
    s.right->setSetPoint(blf::Transform::fromPlanar(0.02, -0.09, -0.04));
    s.com->setSetPoint(blf::Vector3{{0.02, 0.0, 0.45}}, blf::Vector3{{0.0, 0.01, 0.0}});
    s.posture->setSetPoint(blf::VectorXd{0.0, 0.0, -0.2, 0.4, -0.2, 0.0, 0.0, 0.0, -0.2, 0.4, -0.2, 0.0, 0.0});
    const blf::Matrix3 R0 = blf::Transform::fromPlanar(0, 0, 0.1).rotation;
    return ok && s.ik.setRobotState(blf::Vector3{{0.01, -0.02, 0.6}}, R0,
                                    blf::VectorXd{0.02, 0.03, -0.3, 0.6, -0.28, 0.05, -0.03, -0.02, -0.25, 0.5,
                                                  -0.27, -0.04, 0.1});
}

// advance() against the C ABI's solve with the mask `rows` on the adapter's device arrays
static void requireEqualsCAbi(Biped& s, uint32_t rows)
{
    REQUIRE(s.ik.hardRows() == rows);
    REQUIRE(s.ik.advance());
    REQUIRE(s.ik.isValid());
    const IntegrationBasedIKState got = s.ik.get();
    REQUIRE(s.ik.deviceHard().rows == rows);
    blf::DeviceBuffer<double> out(6 + kJoints);
    blf::DeviceBuffer<int32_t> status(1);
    blf_ik_hard hard{};
    hard.rows = rows;
    const blf_status called =
        rows != 0 ? blf_fb_ik_solve_hard(blf::threadHandle(), &s.ik.deviceModel(), &s.ik.deviceState(),
                                         &s.ik.deviceTasks(), &hard, 1, out.data(), status.data(), nullptr)
                  : blf_fb_ik_solve(blf::threadHandle(), &s.ik.deviceModel(), &s.ik.deviceState(),
                                    &s.ik.deviceTasks(), 1, out.data(), status.data(), nullptr);
    REQUIRE(called == BLF_OK);
    std::vector<double> nu;
    std::vector<int32_t> st;
    REQUIRE(out.download(nu) && status.download(st));
    REQUIRE(st[0] == BLF_IK_OK);
    REQUIRE(std::memcmp(nu.data(), got.baseVelocity.data(), 6 * sizeof(double)) == 0);
    REQUIRE(std::memcmp(nu.data() + 6, got.jointVelocity.data(), kJoints * sizeof(double)) == 0);
}

static void testPriorityOnDevice()
{
    Biped s;
    REQUIRE(makeBiped(s));
    requireEqualsCAbi(s, 0u);
    const IntegrationBasedIKState soft = s.ik.get();
    REQUIRE(s.ik.setTaskPriority("left_foot", 0));   // touch-down of the left foot
    requireEqualsCAbi(s, 0x3fu);
    const IntegrationBasedIKState stance = s.ik.get();
    double moved = 0.0;
    for (int i = 0; i < kJoints; ++i) moved = std::max(moved, std::abs(stance.jointVelocity[i] - soft.jointVelocity[i]));
    REQUIRE(moved > 1e-6);   // the hard rows change the solution
    REQUIRE(s.ik.setTaskPriority("right_foot", 0));
    REQUIRE(s.ik.setTaskPriority("com", 0));
    requireEqualsCAbi(s, 0xfffu | (0x7u << 24));
    REQUIRE(s.ik.setTaskPriority("left_foot", 1));   // lift-off
    REQUIRE(s.ik.setTaskPriority("com", 1));
    requireEqualsCAbi(s, 0x3fu << 6);
    REQUIRE(s.ik.setTaskPriority("right_foot", 1));
    requireEqualsCAbi(s, 0u);
    const IntegrationBasedIKState again = s.ik.get();
    REQUIRE(std::memcmp(again.jointVelocity.data(), soft.jointVelocity.data(), kJoints * sizeof(double)) == 0);
    // the weights the tasks were added with are still the ones on the device
    std::vector<double> w(12);
    REQUIRE(hipMemcpy(w.data(), s.ik.deviceTasks().se3_weight, 12 * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess);
    REQUIRE(w[0] == 12.0 && w[5] == 12.0 && w[6] == 9.0 && w[11] == 9.0);
}

int main(int argc, char** argv)
{
    return runCases(argc, argv, {
        {"QPInverseKinematics task priority bookkeeping", false, testPriorityBookkeeping},
        {"QPInverseKinematics task priority on the device", true, testPriorityOnDevice},
    });
}
