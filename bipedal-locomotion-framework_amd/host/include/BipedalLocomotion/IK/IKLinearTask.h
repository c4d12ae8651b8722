/**
 * @file IKLinearTask.h
 * Base of the inverse-kinematics tasks QPInverseKinematics accepts (upstream's IK::IKLinearTask).
 * Upstream's task is a generic linear row block A nu = b evaluated through iDynTree; here the task
 * kinds the device kernel forms itself (include/blf/blf_c.h sections 12 and 12c) are the whole set, so
 * the base only carries the kind and the parameter handling.
 */
#ifndef BLF_BIPEDAL_LOCOMOTION_IK_LINEAR_TASK_H
#define BLF_BIPEDAL_LOCOMOTION_IK_LINEAR_TASK_H

#include <memory>

#include <BipedalLocomotion/ParametersHandler/IParametersHandler.h>

namespace BipedalLocomotion
{
namespace IK
{

class IKLinearTask
{
public:
    enum class Kind
    {
        SE3,
        CoM,
        JointTracking,
        JointLimits
    };
    virtual ~IKLinearTask() = default;
    virtual Kind kind() const = 0;
    /** Read the task's gains; false (with a "[Task::initialize]" line) if a key is missing or bad. */
    virtual bool initialize(std::weak_ptr<ParametersHandler::IParametersHandler> handler) = 0;
    /** True once initialize() succeeded and a set point was given. */
    virtual bool isValid() const = 0;
};

} // namespace IK
} // namespace BipedalLocomotion

#endif // BLF_BIPEDAL_LOCOMOTION_IK_LINEAR_TASK_H
