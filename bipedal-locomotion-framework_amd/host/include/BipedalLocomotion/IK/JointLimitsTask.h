/**
 * @file JointLimitsTask.h
 * Upstream's IK::JointLimitsTask: the joint positions stay inside [lower, upper] through a box on
 * the joint velocities, klim (lower - s) / sampling_time <= sdot <= klim (upper - s) / sampling_time
 * (include/blf/blf_c.h section 12c).  Keys: "klim" (one gain per joint, in (0, 1]), "sampling_time"
 * (> 0), "use_model_limits" (bool) and, when that is false, "lower_limits" and "upper_limits" (one
 * entry per joint, lower <= upper, infinite entries switch a side off); optional "velocity_limits"
 * (one entry per joint, > 0), which intersects the box with [-v, v].  With "use_model_limits" the
 * range is the robot model's (blf::RobotModel::jointLower / jointUpper, which blf::loadUrdf fills),
 * resolved by QPInverseKinematics::finalize().  The task has no set point; QPInverseKinematics takes
 * it at priority 0 only.
 */
#ifndef BLF_BIPEDAL_LOCOMOTION_IK_JOINT_LIMITS_TASK_H
#define BLF_BIPEDAL_LOCOMOTION_IK_JOINT_LIMITS_TASK_H

#include <vector>

#include <BipedalLocomotion/IK/IKLinearTask.h>

namespace BipedalLocomotion
{
namespace IK
{

class JointLimitsTask : public IKLinearTask
{
    bool m_isInitialized{false}, m_useModelLimits{false};
    double m_samplingTime{0.0};
    std::vector<double> m_klim, m_lower, m_upper, m_velocity;

public:
    Kind kind() const final { return Kind::JointLimits; }
    bool initialize(std::weak_ptr<ParametersHandler::IParametersHandler> handler) final;
    bool isValid() const final { return m_isInitialized; }

    bool useModelLimits() const { return m_useModelLimits; }
    double samplingTime() const { return m_samplingTime; }
    const std::vector<double>& klim() const { return m_klim; }
    const std::vector<double>& lowerLimits() const { return m_lower; }      /**< empty with use_model_limits */
    const std::vector<double>& upperLimits() const { return m_upper; }
    const std::vector<double>& velocityLimits() const { return m_velocity; } /**< empty: none */
};

} // namespace IK
} // namespace BipedalLocomotion

#endif // BLF_BIPEDAL_LOCOMOTION_IK_JOINT_LIMITS_TASK_H
