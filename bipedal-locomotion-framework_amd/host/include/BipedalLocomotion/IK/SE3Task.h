/**
 * @file SE3Task.h
 * Upstream's IK::SE3Task: tracks a frame's pose, v* = (v_ff + kp_linear (p_des - p),
 * w_ff + kp_angular Log(R_des R^T)).  Keys: "frame_name" (resolved through the frame names given
 * to QPInverseKinematics::setRobotModel) or "frame_index", "kp_linear", "kp_angular".  The set
 * point is a blf::Transform and a mixed velocity blf::Vector6 (no manif types).  A zero in the
 * weight given to addTask() drops that row: three linear zeros make it upstream's SO3Task, three
 * angular zeros its R3Task.
 */
#ifndef BLF_BIPEDAL_LOCOMOTION_IK_SE3_TASK_H
#define BLF_BIPEDAL_LOCOMOTION_IK_SE3_TASK_H

#include <string>

#include <BipedalLocomotion/IK/IKLinearTask.h>
#include <blf/spatial.h>

namespace BipedalLocomotion
{
namespace IK
{

class SE3Task : public IKLinearTask
{
    bool m_isInitialized{false}, m_hasSetPoint{false};
    std::string m_frameName;
    int m_frameIndex{-1};
    double m_kpLinear{0.0}, m_kpAngular{0.0};
    blf::Transform m_pose;
    blf::Vector6 m_mixedVelocity{};

public:
    Kind kind() const final { return Kind::SE3; }
    bool initialize(std::weak_ptr<ParametersHandler::IParametersHandler> handler) final;
    bool setSetPoint(const blf::Transform& pose, const blf::Vector6& mixedVelocity = blf::Vector6{});
    bool isValid() const final { return m_isInitialized && m_hasSetPoint; }

    const std::string& frameName() const { return m_frameName; }
    int frameIndex() const { return m_frameIndex; }
    double kpLinear() const { return m_kpLinear; }
    double kpAngular() const { return m_kpAngular; }
    const blf::Transform& pose() const { return m_pose; }
    const blf::Vector6& mixedVelocity() const { return m_mixedVelocity; }
};

} // namespace IK
} // namespace BipedalLocomotion

#endif // BLF_BIPEDAL_LOCOMOTION_IK_SE3_TASK_H
