/**
 * @file CoMTask.h
 * Upstream's IK::CoMTask: tracks the centre of mass, v* = cdot_des + kp_linear (c_des - c).
 * Key: "kp_linear".
 */
#ifndef BLF_BIPEDAL_LOCOMOTION_IK_COM_TASK_H
#define BLF_BIPEDAL_LOCOMOTION_IK_COM_TASK_H

#include <BipedalLocomotion/IK/IKLinearTask.h>
#include <blf/spatial.h>

namespace BipedalLocomotion
{
namespace IK
{

class CoMTask : public IKLinearTask
{
    bool m_isInitialized{false}, m_hasSetPoint{false};
    double m_kp{0.0};
    blf::Vector3 m_position{}, m_velocity{};

public:
    Kind kind() const final { return Kind::CoM; }
    bool initialize(std::weak_ptr<ParametersHandler::IParametersHandler> handler) final;
    bool setSetPoint(const blf::Vector3& position, const blf::Vector3& velocity = blf::Vector3{});
    bool isValid() const final { return m_isInitialized && m_hasSetPoint; }

    double kpLinear() const { return m_kp; }
    const blf::Vector3& position() const { return m_position; }
    const blf::Vector3& velocity() const { return m_velocity; }
};

} // namespace IK
} // namespace BipedalLocomotion

#endif // BLF_BIPEDAL_LOCOMOTION_IK_COM_TASK_H
