/**
 * @file ik_limits_tests.cpp
 * Tests of IK::JointLimitsTask in IK::QPInverseKinematics, with ik_tests.cpp's conventions
 * ("name ... ok", "N checks, 0 failed"; modes cpu / gpu / all; `urdf <file>` prints the limits
 * blf::loadUrdf reads, for tests/test_host_ik_limits.py to compare with blf/urdf.py):
 *   cpu: the task's keys and refusals; addTask takes it at priority 0 only, once, without a weight;
 *        blf::loadUrdf's jointLower / jointUpper / jointVelocityLimit follow the fixed-joint merge;
 *   gpu: finalize() refuses a task of the wrong size and "use_model_limits" on a model without
 *        limits (finalize needs the model, which needs a device); on a 13-joint biped with hard feet
 *        advance() equals blf_fb_ik_solve_limits with a bound active, and returns false when the
 *        velocity limits leave the hard feet no solution.
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
#include <blf/urdf.h>

#include "ik_fixtures.h"
#include "test_harness.h"

using namespace BipedalLocomotion;
using namespace BipedalLocomotion::IK;
using namespace BipedalLocomotion::ParametersHandler;

static std::shared_ptr<StdImplementation> limitsHandler(int n = kJoints, double velocity = 0.0)
{
    auto h = std::make_shared<StdImplementation>();
    h->setParameter("klim", std::vector<double>(n, 0.5));
    h->setParameter("sampling_time", 0.01);
    h->setParameter("use_model_limits", false);
    h->setParameter("lower_limits", std::vector<double>(n, -1.0));
    h->setParameter("upper_limits", std::vector<double>(n, 1.0));
    if (velocity > 0.0) h->setParameter("velocity_limits", std::vector<double>(n, velocity));
    return h;
}

static std::shared_ptr<JointLimitsTask> limitsTask(std::shared_ptr<StdImplementation> h = limitsHandler())
{
    auto t = std::make_shared<JointLimitsTask>();
    t->initialize(h);
    return t;
}

static void testLimitsTaskKeys()
{
    JointLimitsTask t;
    REQUIRE_FALSE(t.isValid());
    REQUIRE_FALSE(t.initialize(std::shared_ptr<StdImplementation>()));
    REQUIRE(t.initialize(limitsHandler()));
    REQUIRE(t.isValid() && !t.useModelLimits() && t.samplingTime() == 0.01 && t.klim().size() == kJoints);
    REQUIRE(t.lowerLimits()[0] == -1.0 && t.upperLimits()[kJoints - 1] == 1.0 && t.velocityLimits().empty());
    REQUIRE(t.initialize(limitsHandler(kJoints, 2.0)) && t.velocityLimits().size() == kJoints);
    for (const char* key : {"klim", "sampling_time", "use_model_limits", "lower_limits", "upper_limits"})
    {
        auto h = std::make_shared<StdImplementation>();   // every key but one
        if (std::strcmp(key, "klim")) h->setParameter("klim", std::vector<double>(kJoints, 0.5));
        if (std::strcmp(key, "sampling_time")) h->setParameter("sampling_time", 0.01);
        if (std::strcmp(key, "use_model_limits")) h->setParameter("use_model_limits", false);
        if (std::strcmp(key, "lower_limits")) h->setParameter("lower_limits", std::vector<double>(kJoints, -1.0));
        if (std::strcmp(key, "upper_limits")) h->setParameter("upper_limits", std::vector<double>(kJoints, 1.0));
        REQUIRE_FALSE(t.initialize(h));
        REQUIRE_FALSE(t.isValid());
    }
    for (double bad : {0.0, -0.5, 1.5, static_cast<double>(NAN)})
    {
        auto h = limitsHandler();
        h->setParameter("klim", std::vector<double>(kJoints, bad));
        REQUIRE_FALSE(t.initialize(h));
    }
    for (double bad : {0.0, -0.01, static_cast<double>(NAN), static_cast<double>(INFINITY)})
    {
        auto h = limitsHandler();
        h->setParameter("sampling_time", bad);
        REQUIRE_FALSE(t.initialize(h));
    }
    {
        auto h = limitsHandler();
        h->setParameter("lower_limits", std::vector<double>(kJoints, 2.0));   // above the upper limits
        REQUIRE_FALSE(t.initialize(h));
        h->setParameter("lower_limits", std::vector<double>(kJoints - 1, -1.0));   // wrong size
        REQUIRE_FALSE(t.initialize(h));
        h->setParameter("lower_limits", std::vector<double>(kJoints, static_cast<double>(NAN)));
        REQUIRE_FALSE(t.initialize(h));
        h->setParameter("lower_limits", std::vector<double>(kJoints, -static_cast<double>(INFINITY)));
        REQUIRE(t.initialize(h));                                              // a one-sided range
    }
    for (double bad : {0.0, -1.0, static_cast<double>(NAN)})
    {
        auto h = limitsHandler();
        h->setParameter("velocity_limits", std::vector<double>(kJoints, bad));
        REQUIRE_FALSE(t.initialize(h));
    }
    {
        auto h = limitsHandler();
        h->setParameter("velocity_limits", std::vector<double>(kJoints + 1, 1.0));
        REQUIRE_FALSE(t.initialize(h));
    }
    {
        auto h = std::make_shared<StdImplementation>();   // the model's limits: no arrays needed
        h->setParameter("klim", std::vector<double>(kJoints, 1.0));
        h->setParameter("sampling_time", 0.002);
        h->setParameter("use_model_limits", true);
        REQUIRE(t.initialize(h));
        REQUIRE(t.useModelLimits() && t.lowerLimits().empty());
    }
}

static void testLimitsTaskBookkeeping()
{
    QPInverseKinematics ik;
    REQUIRE_FALSE(ik.addTask(limitsTask(), "limits_soft", 1, blf::VectorXd(kJoints, 1.0)));   // priority 1
    REQUIRE_FALSE(ik.addTask(limitsTask(), "limits_soft", 1));
    REQUIRE_FALSE(ik.addTask(limitsTask(), "limits_low", 2));
    REQUIRE_FALSE(ik.addTask(limitsTask(), "limits_weight", 0, blf::VectorXd(kJoints, 1.0)));  // takes no weight
    REQUIRE(ik.getTaskNames().empty());
    REQUIRE(ik.addTask(limitsTask(), "limits", 0));
    REQUIRE(ik.hardRows() == 0u);                                                             // no task rows
    REQUIRE_FALSE(ik.addTask(limitsTask(), "limits2", 0));                                    // once only
    REQUIRE_FALSE(ik.addTask(limitsTask(), "limits", 0));
    REQUIRE(ik.addTask(se3Task(0), "foot", 0));
    REQUIRE(ik.hardRows() == 0x3fu);
    REQUIRE(ik.getTaskNames().size() == 2);
    REQUIRE_FALSE(ik.advance());                                                              // no joint tracking task
    REQUIRE(ik.addTask(jointTask(), "posture", 1, blf::VectorXd(kJoints, 0.1)));
    REQUIRE_FALSE(ik.advance());                                                              // before finalize
    REQUIRE_FALSE(ik.finalize());                                                             // no robot model
    REQUIRE(ik.deviceLimits().pos_lower == nullptr);
}

static const char* kUrdf = R"(<robot name="r">
  <link name="base"/><link name="a"/><link name="b"/><link name="c"/><link name="d"/><link name="e"/>
  <joint name="rev" type="revolute"><parent link="base"/><child link="a"/><axis xyz="0 1 0"/>
    <limit lower="-0.5" upper="1.25" velocity="3.0" effort="10"/></joint>
  <joint name="weld" type="fixed"><parent link="a"/><child link="b"/><limit lower="-9" upper="9" velocity="9"/></joint>
  <joint name="cont" type="continuous"><parent link="b"/><child link="c"/><axis xyz="0 0 1"/>
    <limit lower="-1" upper="1" velocity="2.5"/></joint>
  <joint name="slide" type="prismatic"><parent link="c"/><child link="d"/><axis xyz="1 0 0"/>
    <limit lower="0.0" upper="0.3"/></joint>
  <joint name="bare" type="revolute"><parent link="d"/><child link="e"/><axis xyz="1 0 0"/></joint>
</robot>)";

static void testUrdfLimits()
{
    blf::RobotModel m;
    std::vector<std::string> names;
    std::string err;
    REQUIRE(blf::loadUrdf(kUrdf, blf::UrdfOptions{}, m, &names, &err));
    REQUIRE(m.ndof == 4 && names.size() == 4 && names[0] == "rev" && names[1] == "cont" && names[3] == "bare");
    REQUIRE(m.jointLower.size() == 4 && m.jointUpper.size() == 4 && m.jointVelocityLimit.size() == 4);
    REQUIRE(m.jointLower[0] == -0.5 && m.jointUpper[0] == 1.25 && m.jointVelocityLimit[0] == 3.0);
    REQUIRE(m.jointLower[1] == -HUGE_VAL && m.jointUpper[1] == HUGE_VAL && m.jointVelocityLimit[1] == 2.5);
    REQUIRE(m.jointLower[2] == 0.0 && m.jointUpper[2] == 0.3 && m.jointVelocityLimit[2] == HUGE_VAL);
    REQUIRE(m.jointLower[3] == -HUGE_VAL && m.jointUpper[3] == HUGE_VAL && m.jointVelocityLimit[3] == HUGE_VAL);
    blf::UrdfOptions two;   // the others locked, the order reversed
    two.hasConsideredJoints = true;
    two.consideredJoints = {"rev", "slide"};
    REQUIRE(blf::loadUrdf(kUrdf, two, m, &names, &err));
    REQUIRE(m.ndof == 2 && m.jointLower.size() == 2 && m.jointLower[1] == 0.0 && m.jointUpper[0] == 1.25);
    std::string bad(kUrdf);
    bad.replace(bad.find("lower=\"-0.5\""), 12, "lower=\"2.5\" ");
    REQUIRE_FALSE(blf::loadUrdf(bad, blf::UrdfOptions{}, m, &names, &err));
    REQUIRE(err.find("lower limit") != std::string::npos);
}

static int dumpUrdfLimits(const char* path)
{
    blf::RobotModel m;
    std::vector<std::string> names;
    std::string err;
    if (!blf::loadUrdf(path, blf::UrdfOptions{}, m, &names, &err))
    {
        std::fprintf(stderr, "%s\n", err.c_str());
        return 1;
    }
    for (int j = 0; j < m.ndof; ++j)
        std::printf("%s %.17g %.17g %.17g\n", names[j].c_str(), m.jointLower[j], m.jointUpper[j],
                    m.jointVelocityLimit[j]);
    return 0;
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
    std::shared_ptr<JointLimitsTask> limits;
};

// The standing set with hard feet, the CoM and the posture weighted, and the joint limits.
static bool makeBiped(Biped& s, std::shared_ptr<JointLimitsTask> limits, const blf::RobotModel& model = bipedModel(),
                      bool finalize = true)
{
    auto h = std::make_shared<StdImplementation>();
    h->setParameter("hard_task_weight", 20.0);
    bool ok = s.ik.initialize(h);
    ok = ok && s.ik.setRobotModel(model, {"l_sole", "r_sole"});
    s.left = se3Task(0);
    s.right = se3Task(1);
    s.com = comTask();
    s.posture = jointTask();
    s.limits = limits;
    ok = ok && s.ik.addTask(s.left, "left_foot", 0);
    ok = ok && s.ik.addTask(s.right, "right_foot", 0);
    ok = ok && s.ik.addTask(s.com, "com", 1, blf::VectorXd(3, 10.0));
    ok = ok && s.ik.addTask(s.posture, "posture", 1, blf::VectorXd(kJoints, 0.1));
    ok = ok && s.ik.addTask(s.limits, "limits", 0);
    if (!finalize) return ok;
    ok = ok && s.ik.finalize();
    s.left->setSetPoint(blf::Transform::fromPlanar(0.03, 0.09, 0.05), blf::Vector6{{0.01, 0, 0, 0, 0, 0.02}});
    s.right->setSetPoint(blf::Transform::fromPlanar(0.02, -0.09, -0.04));
    s.com->setSetPoint(blf::Vector3{{0.02, 0.0, 0.45}}, blf::Vector3{{0.0, 0.01, 0.0}});
    s.posture->setSetPoint(blf::VectorXd{0.0, 0.0, -0.2, 0.4, -0.2, 0.0, 0.0, 0.0, -0.2, 0.4, -0.2, 0.0, 0.0});
    const blf::Matrix3 R0 = blf::Transform::fromPlanar(0, 0, 0.1).rotation;
    return ok && s.ik.setRobotState(kBase0, R0, joints0());
}

static void testFinalizeRefusals()
{
    {
        Biped s;   // twelve gains for thirteen joints
        REQUIRE(makeBiped(s, limitsTask(limitsHandler(kJoints - 1)), bipedModel(), false));
        REQUIRE_FALSE(s.ik.finalize());
    }
    auto model = std::make_shared<StdImplementation>();
    model->setParameter("klim", std::vector<double>(kJoints, 0.5));
    model->setParameter("sampling_time", 0.01);
    model->setParameter("use_model_limits", true);
    {
        Biped s;   // the model has no limits
        REQUIRE(makeBiped(s, limitsTask(model), bipedModel(), false));
        REQUIRE_FALSE(s.ik.finalize());
    }
    {
        Biped s;   // it has them now
        blf::RobotModel m = bipedModel();
        m.jointLower.assign(kJoints, -1.5);
        m.jointUpper.assign(kJoints, 1.5);
        REQUIRE(makeBiped(s, limitsTask(model), m));
        REQUIRE(s.ik.advance());
        REQUIRE(s.ik.deviceLimits().pos_lower != nullptr && s.ik.deviceLimits().vel_max == nullptr
                && s.ik.deviceLimits().sampling_time == 0.01);
    }
    {
        Biped s;   // lower and upper limits of different sizes: a corrupted model
        blf::RobotModel m = bipedModel();
        m.jointLower.assign(kJoints, -1.5);
        auto h = std::make_shared<StdImplementation>();
        REQUIRE(s.ik.initialize(h));
        REQUIRE_FALSE(s.ik.setRobotModel(m, {"l_sole", "r_sole"}));
    }
}

static void testLimitsOnDevice()
{
    Biped free, held;
    REQUIRE(makeBiped(free, limitsTask(limitsHandler(kJoints, 100.0))));
    REQUIRE(free.ik.advance());
    // a velocity limit at 0.6 of the largest joint speed without limits: some joint ends on it
    double top = 0.0;
    for (int i = 0; i < kJoints; ++i) top = std::max(top, std::abs(free.ik.get().jointVelocity[i]));
    REQUIRE(top > 1e-3);
    const double vmax = 0.6 * top;
    REQUIRE(makeBiped(held, limitsTask(limitsHandler(kJoints, vmax))));
    REQUIRE(held.ik.advance());
    REQUIRE(held.ik.isValid());
    const IntegrationBasedIKState got = held.ik.get();
    int onBound = 0;
    for (int i = 0; i < kJoints; ++i)
    {
        REQUIRE(std::abs(got.jointVelocity[i]) <= vmax + 1e-12);
        onBound += std::abs(got.jointVelocity[i]) == vmax;
    }
    REQUIRE(onBound >= 1);
    // the same solve through the C ABI, on the adapter's device arrays
    blf::DeviceBuffer<double> out(6 + kJoints);
    blf::DeviceBuffer<int32_t> status(1), iters(1);
    blf::DeviceBuffer<double> active(2);   // two 64-bit words (DeviceBuffer has no uint64_t form)
    REQUIRE(blf_fb_ik_solve_limits(blf::threadHandle(), &held.ik.deviceModel(), &held.ik.deviceState(),
                                   &held.ik.deviceTasks(), &held.ik.deviceHard(), &held.ik.deviceLimits(), 1,
                                   out.data(), status.data(), iters.data(), reinterpret_cast<uint64_t*>(active.data()),
                                   nullptr) == BLF_OK);
    std::vector<double> nu;
    std::vector<int32_t> st, it;
    std::vector<double> words;
    REQUIRE(out.download(nu) && status.download(st) && iters.download(it) && active.download(words));
    uint64_t act[2] = {0, 0};
    std::memcpy(act, words.data(), sizeof(act));
    REQUIRE(st[0] == BLF_IK_OK && it[0] >= 2 && (act[0] | act[1]) != 0);
    REQUIRE(std::memcmp(nu.data(), got.baseVelocity.data(), 6 * sizeof(double)) == 0);
    REQUIRE(std::memcmp(nu.data() + 6, got.jointVelocity.data(), kJoints * sizeof(double)) == 0);
}

static void testInfeasibleLimitsOnDevice()
{
    Biped s;   // the hard feet ask for motion the velocity limits forbid
    REQUIRE(makeBiped(s, limitsTask(limitsHandler(kJoints, 1e-6))));
    REQUIRE_FALSE(s.ik.advance());
    REQUIRE_FALSE(s.ik.isValid());
}

int main(int argc, char** argv)
{
    if (argc > 2 && std::strcmp(argv[1], "urdf") == 0) return dumpUrdfLimits(argv[2]);
    return runCases(argc, argv, {
        {"JointLimitsTask keys", false, testLimitsTaskKeys},
        {"QPInverseKinematics limits task bookkeeping", false, testLimitsTaskBookkeeping},
        {"loadUrdf joint limits", false, testUrdfLimits},
        {"QPInverseKinematics limits finalize", true, testFinalizeRefusals},
        {"QPInverseKinematics limits on the device", true, testLimitsOnDevice},
        {"QPInverseKinematics infeasible limits", true, testInfeasibleLimitsOnDevice},
    });
}
