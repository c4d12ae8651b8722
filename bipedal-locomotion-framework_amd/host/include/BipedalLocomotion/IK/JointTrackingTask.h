/**
 * @file JointTrackingTask.h
 * Upstream's IK::JointTrackingTask: sdot* = sdot_des + kp (s_des - s), the posture regulariser
 * that makes the IK's normal matrix positive definite.  Key: "kp" (one gain per joint).
 */
#ifndef BLF_BIPEDAL_LOCOMOTION_IK_JOINT_TRACKING_TASK_H
#define BLF_BIPEDAL_LOCOMOTION_IK_JOINT_TRACKING_TASK_H

#include <vector>

#include <BipedalLocomotion/IK/IKLinearTask.h>
#include <blf/dense.h>

namespace BipedalLocomotion
{
namespace IK
{

class JointTrackingTask : public IKLinearTask
{
    bool m_isInitialized{false}, m_hasSetPoint{false};
    std::vector<double> m_kp;
    blf::VectorXd m_position, m_velocity;

public:
    Kind kind() const final { return Kind::JointTracking; }
    bool initialize(std::weak_ptr<ParametersHandler::IParametersHandler> handler) final;
    /** Desired joint positions with zero desired velocity. */
    bool setSetPoint(const blf::VectorXd& jointPosition);
    bool setSetPoint(const blf::VectorXd& jointPosition, const blf::VectorXd& jointVelocity);
    bool isValid() const final { return m_isInitialized && m_hasSetPoint; }

    const std::vector<double>& kp() const { return m_kp; }
    const blf::VectorXd& position() const { return m_position; }
    const blf::VectorXd& velocity() const { return m_velocity; }
};

} // namespace IK
} // namespace BipedalLocomotion

#endif // BLF_BIPEDAL_LOCOMOTION_IK_JOINT_TRACKING_TASK_H
