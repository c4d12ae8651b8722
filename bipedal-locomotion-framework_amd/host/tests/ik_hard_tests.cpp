/**
 * @file ik_hard_tests.cpp
 * Tests of IK::QPInverseKinematics' hard (priority 0) tasks, with ik_tests.cpp's conventions
 * ("name ... ok", "N checks, 0 failed"; modes cpu / gpu / all):
 *   cpu: addTask with priority 0 accepted without a weight for an SE3Task and a CoMTask, refused
 *        with one and for the JointTrackingTask; "hard_task_weight" out of range; the mask the
 *        adapter builds (hardRows());
 *   gpu: on a 13-joint biped with hard feet, advance() equals blf_fb_ik_solve_hard and differs from
 *        the weighted solve of the same arrays; two hard tasks on one frame make advance() return
 *        false.
 */
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include <BipedalLocomotion/IK/QPInverseKinematics.h>
#include <BipedalLocomotion/ParametersHandler/IParametersHandler.h>

#include "ik_fixtures.h"
#include "test_harness.h"

using namespace BipedalLocomotion;
using namespace BipedalLocomotion::IK;
using namespace BipedalLocomotion::ParametersHandler;

static void testHardTaskBookkeeping()
{
    const blf::VectorXd w6(6, 10.0), w3(3, 5.0), wn(kJoints, 0.1);
    {
        QPInverseKinematics ik;
        auto h = std::make_shared<StdImplementation>();
        REQUIRE(ik.initialize(h));   // hard_task_weight is optional
        for (double bad : {0.0, -1.0, static_cast<double>(NAN), static_cast<double>(INFINITY)})
        {
            h->setParameter("hard_task_weight", bad);
            REQUIRE_FALSE(ik.initialize(h));
        }
        h->setParameter("hard_task_weight", 25.0);
        REQUIRE(ik.initialize(h));
    }
    {
        QPInverseKinematics ik;
        REQUIRE(ik.hardRows() == 0u);
        REQUIRE_FALSE(ik.addTask(se3Task(0), "weighted_hard", 0, w6));   // a hard task takes no weight
        REQUIRE_FALSE(ik.addTask(comTask(), "weighted_hard_com", 0, w3));
        REQUIRE_FALSE(ik.addTask(jointTask(), "hard_posture", 0));       // the regulariser cannot be hard
        REQUIRE_FALSE(ik.addTask(jointTask(), "hard_posture_w", 0, wn));
        REQUIRE_FALSE(ik.addTask(se3Task(0), "low", 2));
        REQUIRE_FALSE(ik.addTask(nullptr, "null", 0));
        REQUIRE(ik.getTaskNames().empty() && ik.hardRows() == 0u);
        REQUIRE(ik.addTask(se3Task(0), "soft_left", 1, w6));             // SE3 task 0: weighted
        REQUIRE(ik.hardRows() == 0u);
        REQUIRE(ik.addTask(se3Task(1), "hard_right", 0));                // SE3 task 1: bits 6..11
        REQUIRE(ik.hardRows() == 0xfc0u);
        REQUIRE_FALSE(ik.addTask(se3Task(1), "hard_right", 0));          // duplicate name
        REQUIRE(ik.addTask(comTask(), "com", 0));                        // bits 24..26
        REQUIRE(ik.hardRows() == (0xfc0u | (7u << 24)));
        REQUIRE_FALSE(ik.addTask(comTask(), "com2", 0));                 // a second CoM task
        REQUIRE_FALSE(ik.addTask(comTask(), "com3", 1, w3));
        REQUIRE(ik.addTask(se3Task(0), "soft_third", 1, w6));
        REQUIRE(ik.addTask(se3Task(1), "hard_fourth", 0));               // SE3 task 3: bits 18..23
        REQUIRE(ik.hardRows() == (0xfc0u | (0x3fu << 18) | (7u << 24)));
        REQUIRE_FALSE(ik.addTask(se3Task(1), "fifth", 0));               // BLF_IK_MAX_SE3_TASKS
        REQUIRE_FALSE(ik.advance());                                     // no joint tracking task
        REQUIRE(ik.addTask(jointTask(), "posture", 1, wn));
        REQUIRE(ik.getTaskNames().size() == 6);
        REQUIRE_FALSE(ik.advance());                                     // before finalize
        REQUIRE_FALSE(ik.finalize());                                    // no robot model
    }
    {
        QPInverseKinematics ik;   // the CoM alone
        REQUIRE(ik.addTask(comTask(), "com", 0));
        REQUIRE(ik.hardRows() == (7u << 24));
    }
}

// ---- device cases ----------------------------------------------------------------------------------
static const blf::Vector3 kBase0{{0.01, -0.02, 0.6}};
static blf::VectorXd joints0()
{
    return blf::VectorXd{0.02, 0.03, -0.3, 0.6, -0.28, 0.05, -0.03, -0.02, -0.25, 0.5, -0.27, -0.04, 0.1};
}

struct Biped
{
    QPInverseKinematics ik;
    std::shared_ptr<SE3Task> left, right;
    std::shared_ptr<CoMTask> com;
    std::shared_ptr<JointTrackingTask> posture;
};

// The standing set: the feet hard (12 rows against 19 unknowns) or weighted, the CoM and the
// posture weighted.
static bool makeBiped(Biped& s, bool hardFeet, int rightFrame = 1)
{
    auto h = std::make_shared<StdImplementation>();
    h->setParameter("hard_task_weight", 20.0);
    bool ok = s.ik.initialize(h);
    ok = ok && s.ik.setRobotModel(bipedModel(), {"l_sole", "r_sole"});
    s.left = se3Task(0);
    s.right = se3Task(rightFrame);
    s.com = comTask();
    s.posture = jointTask();
    if (hardFeet)
    {
        ok = ok && s.ik.addTask(s.left, "left_foot", 0);
        ok = ok && s.ik.addTask(s.right, "right_foot", 0);
    }
    else
    {
        ok = ok && s.ik.addTask(s.left, "left_foot", 1, blf::VectorXd(6, 20.0));
        ok = ok && s.ik.addTask(s.right, "right_foot", 1, blf::VectorXd(6, 20.0));
    }
    ok = ok && s.ik.addTask(s.com, "com", 1, blf::VectorXd(3, 10.0));
    ok = ok && s.ik.addTask(s.posture, "posture", 1, blf::VectorXd(kJoints, 0.1));
    ok = ok && s.ik.finalize();
    s.left->setSetPoint(blf::Transform::fromPlanar(0.03, 0.09, 0.05), blf::Vector6{{0.01, 0, 0, 0, 0, 0.02}});
    s.right->setSetPoint(blf::Transform::fromPlanar(0.02, -0.09, -0.04));
    s.com->setSetPoint(blf::Vector3{{0.02, 0.0, 0.45}}, blf::Vector3{{0.0, 0.01, 0.0}});
    s.posture->setSetPoint(blf::VectorXd{0.0, 0.0, -0.2, 0.4, -0.2, 0.0, 0.0, 0.0, -0.2, 0.4, -0.2, 0.0, 0.0});
    const blf::Matrix3 R0 = blf::Transform::fromPlanar(0, 0, 0.1).rotation;
    return ok && s.ik.setRobotState(kBase0, R0, joints0());
}

static void testHardFeetOnDevice()
{
    Biped hard, soft;
    REQUIRE(makeBiped(hard, true));
    REQUIRE(makeBiped(soft, false));
    REQUIRE(hard.ik.hardRows() == 0xfffu);
    REQUIRE(hard.ik.advance());
    REQUIRE(hard.ik.isValid());
    REQUIRE(hard.ik.deviceHard().rows == 0xfffu && hard.ik.deviceHard().reserved == 0
            && hard.ik.deviceHard().rel_pivot_min == 0.0);
    const IntegrationBasedIKState got = hard.ik.get();
    // the same solve through the C ABI, on the adapter's device arrays
    blf::DeviceBuffer<double> out(6 + kJoints);
    blf::DeviceBuffer<int32_t> status(1);
    REQUIRE(blf_fb_ik_solve_hard(blf::threadHandle(), &hard.ik.deviceModel(), &hard.ik.deviceState(),
                                 &hard.ik.deviceTasks(), &hard.ik.deviceHard(), 1, out.data(), status.data(),
                                 nullptr) == BLF_OK);
    std::vector<double> nu;
    std::vector<int32_t> st;
    REQUIRE(out.download(nu) && status.download(st));
    REQUIRE(st[0] == BLF_IK_OK);
    REQUIRE(std::memcmp(nu.data(), got.baseVelocity.data(), 6 * sizeof(double)) == 0);
    REQUIRE(std::memcmp(nu.data() + 6, got.jointVelocity.data(), kJoints * sizeof(double)) == 0);
    // the hard set's weights are "hard_task_weight"; with the same weights the soft solve differs
    REQUIRE(soft.ik.advance());
    REQUIRE(soft.ik.deviceHard().rows == 0u);
    double diff = 0.0;
    for (int i = 0; i < kJoints; ++i)
        diff = std::max(diff, std::abs(soft.ik.get().jointVelocity[i] - got.jointVelocity[i]));
    REQUIRE(std::isfinite(diff) && diff > 1e-6);
    // the soft solve of the hard adapter's arrays is the soft adapter's, bit for bit (same weights)
    REQUIRE(blf_fb_ik_solve(blf::threadHandle(), &hard.ik.deviceModel(), &hard.ik.deviceState(),
                            &hard.ik.deviceTasks(), 1, out.data(), nullptr, nullptr) == BLF_OK);
    REQUIRE(out.download(nu));
    REQUIRE(std::memcmp(nu.data() + 6, soft.ik.get().jointVelocity.data(), kJoints * sizeof(double)) == 0);
}

static void testDependentHardTasksOnDevice()
{
    Biped s;
    REQUIRE(makeBiped(s, true, 0));   // both hard tasks on the left sole
    REQUIRE_FALSE(s.ik.advance());
    REQUIRE_FALSE(s.ik.isValid());
}

int main(int argc, char** argv)
{
    return runCases(argc, argv, {
        {"QPInverseKinematics hard task bookkeeping", false, testHardTaskBookkeeping},
        {"QPInverseKinematics hard feet on the device", true, testHardFeetOnDevice},
        {"QPInverseKinematics dependent hard tasks", true, testDependentHardTasksOnDevice},
    });
}
