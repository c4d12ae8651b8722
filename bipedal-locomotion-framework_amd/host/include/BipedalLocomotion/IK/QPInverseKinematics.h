/**
 * @file QPInverseKinematics.h
 * Upstream's IK::QPInverseKinematics over SE3Task, CoMTask and JointTrackingTask, for one robot:
 * advance() solves for the generalized velocity nu = (base mixed twist, joint velocities) that
 * minimises the weighted task errors at the robot state, on the device (blf_fb_ik_solve,
 * include/blf/blf_c.h section 12), subject to the hard (priority 0) tasks holding exactly
 * (blf_fb_ik_solve_hard, section 12b) and to the joint limits of a JointLimitsTask
 * (blf_fb_ik_solve_limits, section 12c).  Integrating that velocity with
 * ForwardEuler<FloatingBaseSystemKinematics> and feeding the state back with setRobotState() is
 * upstream's IntegrationBasedIK loop; blf_fb_ik_integrate(_hard) runs the same loop in one launch.
 *
 * Differences from upstream a user can notice: priority 0 (hard) is for SE3Task and CoMTask only
 * and always covers every row of the task (a mask over single rows is the C ABI's); hard tasks that
 * are linearly dependent, conflicting or more than 6 + n rows make advance() return false instead
 * of leaving the choice to a QP solver; the only inequality task is JointLimitsTask (priority 0,
 * once), solved by section 12c's active-set iteration, which is not a complete QP solver: where the
 * limits contradict the hard tasks, and in rare barely feasible cases, advance() returns false
 * (BLF_IK_LIMITS_UNRESOLVED) where a QP solver would report infeasibility or find the point; there
 * are no priorities above 1; at
 * most BLF_IK_MAX_SE3_TASKS SE3 tasks, one CoM task and one joint
 * tracking task, which is required and weighted (it makes the problem positive definite); the robot is a
 * blf::RobotModel set with setRobotModel() (no iDynTree KinDynComputations) and its state is given
 * with setRobotState(); set points and the state hold blf::Transform / blf::Vector6 (no manif
 * types); the optional key "base_damping" (default 0) is added to the base diagonal; the optional
 * key "hard_task_weight" (default 1) is the weight a hard task's rows enter H with, which
 * conditions the factorization and does not change the solution.
 */
#ifndef BLF_BIPEDAL_LOCOMOTION_IK_QP_INVERSE_KINEMATICS_H
#define BLF_BIPEDAL_LOCOMOTION_IK_QP_INVERSE_KINEMATICS_H

#include <memory>
#include <string>
#include <vector>

#include <BipedalLocomotion/IK/CoMTask.h>
#include <BipedalLocomotion/IK/IKLinearTask.h>
#include <BipedalLocomotion/IK/JointLimitsTask.h>
#include <BipedalLocomotion/IK/JointTrackingTask.h>
#include <BipedalLocomotion/IK/SE3Task.h>
#include <BipedalLocomotion/System/Advanceable.h>
#include <blf/dense.h>
#include <blf/device.h>
#include <blf/robot_model.h>
#include <blf/spatial.h>

namespace BipedalLocomotion
{
namespace IK
{

struct IntegrationBasedIKState
{
    blf::VectorXd jointVelocity;
    blf::Vector6 baseVelocity{};   /**< (linear, angular), mixed representation */
};

class QPInverseKinematics : public System::Advanceable<IntegrationBasedIKState>
{
public:
    /** Optional keys "base_damping" (finite, >= 0; default 0) and "hard_task_weight" (finite, > 0;
     * default 1; read by the addTask() calls that follow).  False if the handler is expired or a
     * value is out of range. */
    bool initialize(std::weak_ptr<ParametersHandler::IParametersHandler> handler);

    /** The robot (replaces upstream's KinDynComputations) and, optionally, the names of its frames
     * (frameNames[i] names model.frameLink[i]; what SE3Task's "frame_name" is resolved through).
     * Fixed joints are merged as FloatingBaseDynamicalSystem::setRobotModel does.  Needs a device. */
    bool setRobotModel(const blf::RobotModel& model, const std::vector<std::string>& frameNames = {});

    /** The state the next advance() solves at. */
    bool setRobotState(const blf::Vector3& basePosition, const blf::Matrix3& baseRotation,
                       const blf::VectorXd& jointPositions);

    /**
     * Add a task.  Priority 1 (weighted): weight holds one entry per task row (SE3: 6, linear xyz
     * then angular xyz; CoM: 3; joint tracking: one per joint, > 0), each finite and >= 0.
     * Priority 0 (hard: every row of the task holds exactly): an SE3Task or a CoMTask, with an
     * empty weight; or the JointLimitsTask (priority 0 only, once, empty weight).
     * False with a "[QPInverseKinematics::addTask] ..." line for any other
     * priority, priority 0 with a weight or for a JointTrackingTask, a null task, a duplicate name,
     * a wrong weight, a fifth SE3 task, a second CoM or joint tracking task, or after finalize().
     */
    bool addTask(std::shared_ptr<IKLinearTask> task, const std::string& taskName, unsigned int priority,
                 const blf::VectorXd& weight = blf::VectorXd());

    std::vector<std::string> getTaskNames() const;

    /**
     * Switch a task between weighted (1) and hard (0), also after finalize() and between advance()
     * calls (the task set itself stays fixed): the adapter's form of a contact flag (a stance foot's task is hard, a swing foot's weighted; the
     * batched form is blf_fb_ik_track's schedule, section 12d).  For an SE3Task or a CoMTask that was
     * added at priority 1 with every weight > 0: while hard its rows hold exactly and enter H with
     * the weights it was added with.  hardRows() reflects the switch.  False with a
     * "[QPInverseKinematics::setTaskPriority] ..." line for an unknown name, a
     * priority above 1, a task of another kind, one that was added at priority 0, or one with a zero
     * weight; the task then keeps its priority.
     */
    bool setTaskPriority(const std::string& taskName, unsigned int priority);

    /** Resolve the frames and fix the task set; false without a model or with an unknown frame, or
     * when the JointLimitsTask's sizes do not match the model or it asks for the model's limits
     * ("use_model_limits") and the model has none. */
    bool finalize();

    /** Solve at the robot state with the tasks' current set points.  False before finalize() or
     * setRobotState(), without a joint tracking task, when a task has no set point or a wrong size,
     * or when the device reports a failed solve, dependent hard tasks (BLF_IK_HARD_DEPENDENT) and
     * joint limits the iteration could not resolve (BLF_IK_LIMITS_UNRESOLVED) among them (the
     * state is then invalid). */
    bool advance() final;
    const IntegrationBasedIKState& get() const final { return m_state; }
    bool isValid() const final { return m_isValid; }

    /** The device-side description of the last advance() (for callers that go on with
     * blf_fb_ik_integrate): valid until the next advance(). */
    const blf_fb_model& deviceModel() const { return m_cModel; }
    const blf_fb_state& deviceState() const { return m_cState; }
    const blf_ik_tasks& deviceTasks() const { return m_cTasks; }
    const blf_ik_hard& deviceHard() const { return m_cHard; }
    /** The limits of the last advance(); every pointer is null without a JointLimitsTask. */
    const blf_ik_limits& deviceLimits() const { return m_cLimits; }

    /** Section 12b's mask of the tasks that are hard now: bits 6k..6k+5 for the k-th SE3 task (in
     * the order they were added) when it is hard, bits 24..26 for a hard CoM task. */
    uint32_t hardRows() const;

private:
    struct Entry
    {
        std::string name;
        std::shared_ptr<IKLinearTask> task;
        std::vector<double> weight;
        bool hard;
        bool weighted{false};   // added at priority 1 (what setTaskPriority() may switch)
    };
    std::vector<Entry> m_tasks;
    std::vector<int32_t> m_frames;
    int m_comTask{-1}, m_jointTask{-1}, m_limitsTask{-1};
    std::vector<double> m_limits;   // finalize(): pos_lower n | pos_upper n | klim n | vel_max n (or none)
    bool m_isFinalized{false}, m_hasModel{false}, m_hasState{false}, m_isValid{false};
    double m_baseDamping{0.0}, m_hardWeight{1.0};
    blf::DeviceRobotModel m_model;
    std::vector<std::string> m_frameNames;
    blf::Vector3 m_basePosition{};
    blf::Matrix3 m_baseRotation{};
    blf::VectorXd m_jointPositions;
    IntegrationBasedIKState m_state;

    blf::DeviceBuffer<int32_t> m_dInt;
    blf::DeviceBuffer<double> m_dData;
    blf_fb_model m_cModel{};
    blf_fb_state m_cState{};
    blf_ik_tasks m_cTasks{};
    blf_ik_hard m_cHard{};
    blf_ik_limits m_cLimits{};
    blf::DeviceBuffer<double> m_dLimits;
};

} // namespace IK
} // namespace BipedalLocomotion

#endif // BLF_BIPEDAL_LOCOMOTION_IK_QP_INVERSE_KINEMATICS_H
