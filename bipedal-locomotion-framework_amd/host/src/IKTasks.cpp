/**
 * @file IKTasks.cpp
 * Parameter handling and set points of IK::SE3Task, IK::CoMTask and IK::JointTrackingTask, with
 * return values and messages in the library's convention.  The tasks hold data only: the rows are
 * formed on the device by blf_fb_ik_solve (QPInverseKinematics.cpp).
 */
#include <cmath>
#include <iostream>

#include <BipedalLocomotion/IK/CoMTask.h>
#include <BipedalLocomotion/IK/JointLimitsTask.h>
#include <BipedalLocomotion/IK/JointTrackingTask.h>
#include <BipedalLocomotion/IK/SE3Task.h>

using namespace BipedalLocomotion::IK;
using namespace BipedalLocomotion::ParametersHandler;

namespace
{
bool gain(const IParametersHandler& handler, const char* where, const char* key, double& value)
{
    if (!handler.getParameter(key, value))
    {
        std::cerr << "[" << where << "] The parameter " << key << " is missing." << std::endl;
        return false;
    }
    if (!std::isfinite(value) || value < 0.0)
    {
        std::cerr << "[" << where << "] The parameter " << key << " must be a non-negative number."
                  << std::endl;
        return false;
    }
    return true;
}

template <typename Array> bool allFinite(const Array& a, std::size_t n)
{
    for (std::size_t i = 0; i < n; ++i)
        if (!std::isfinite(a[i])) return false;
    return true;
}
} // namespace

bool SE3Task::initialize(std::weak_ptr<IParametersHandler> handlerWeak)
{
    m_isInitialized = false;
    auto handler = handlerWeak.lock();
    if (handler == nullptr)
    {
        std::cerr << "[SE3Task::initialize] The parameters handler no longer exists." << std::endl;
        return false;
    }
    std::string name;
    int index = -1;
    const bool hasName = handler->getParameter("frame_name", name) && !name.empty();
    const bool hasIndex = handler->getParameter("frame_index", index);
    if (!hasName && !hasIndex)
    {
        std::cerr << "[SE3Task::initialize] The parameter frame_name (or frame_index) is missing."
                  << std::endl;
        return false;
    }
    if (!hasName && index < 0)
    {
        std::cerr << "[SE3Task::initialize] The frame_index must be non-negative." << std::endl;
        return false;
    }
    double kpLinear = 0.0, kpAngular = 0.0;
    if (!gain(*handler, "SE3Task::initialize", "kp_linear", kpLinear)
        || !gain(*handler, "SE3Task::initialize", "kp_angular", kpAngular))
        return false;
    m_frameName = hasName ? name : std::string();
    m_frameIndex = hasName ? -1 : index;
    m_kpLinear = kpLinear;
    m_kpAngular = kpAngular;
    m_isInitialized = true;
    return true;
}

bool SE3Task::setSetPoint(const blf::Transform& pose, const blf::Vector6& mixedVelocity)
{
    if (!allFinite(pose.position, 3) || !allFinite(pose.rotation, 9) || !allFinite(mixedVelocity, 6))
    {
        std::cerr << "[SE3Task::setSetPoint] The set point is not finite." << std::endl;
        return false;
    }
    m_pose = pose;
    m_mixedVelocity = mixedVelocity;
    m_hasSetPoint = true;
    return true;
}

bool CoMTask::initialize(std::weak_ptr<IParametersHandler> handlerWeak)
{
    m_isInitialized = false;
    auto handler = handlerWeak.lock();
    if (handler == nullptr)
    {
        std::cerr << "[CoMTask::initialize] The parameters handler no longer exists." << std::endl;
        return false;
    }
    double kp = 0.0;
    if (!gain(*handler, "CoMTask::initialize", "kp_linear", kp)) return false;
    m_kp = kp;
    m_isInitialized = true;
    return true;
}

bool CoMTask::setSetPoint(const blf::Vector3& position, const blf::Vector3& velocity)
{
    if (!allFinite(position, 3) || !allFinite(velocity, 3))
    {
        std::cerr << "[CoMTask::setSetPoint] The set point is not finite." << std::endl;
        return false;
    }
    m_position = position;
    m_velocity = velocity;
    m_hasSetPoint = true;
    return true;
}

bool JointTrackingTask::initialize(std::weak_ptr<IParametersHandler> handlerWeak)
{
    m_isInitialized = false;
    auto handler = handlerWeak.lock();
    if (handler == nullptr)
    {
        std::cerr << "[JointTrackingTask::initialize] The parameters handler no longer exists."
                  << std::endl;
        return false;
    }
    std::vector<double> kp;
    if (!handler->getParameter("kp", kp) || kp.empty())
    {
        std::cerr << "[JointTrackingTask::initialize] The parameter kp is missing." << std::endl;
        return false;
    }
    for (const double k : kp)
        if (!std::isfinite(k) || k < 0.0)
        {
            std::cerr << "[JointTrackingTask::initialize] The gains kp must be non-negative numbers."
                      << std::endl;
            return false;
        }
    m_kp = kp;
    m_isInitialized = true;
    return true;
}

bool JointTrackingTask::setSetPoint(const blf::VectorXd& jointPosition)
{
    return setSetPoint(jointPosition, blf::VectorXd(jointPosition.size(), 0.0));
}

bool JointTrackingTask::setSetPoint(const blf::VectorXd& jointPosition, const blf::VectorXd& jointVelocity)
{
    if (!m_isInitialized)
    {
        std::cerr << "[JointTrackingTask::setSetPoint] The task is not initialized." << std::endl;
        return false;
    }
    if (jointPosition.size() != m_kp.size() || jointVelocity.size() != m_kp.size())
    {
        std::cerr << "[JointTrackingTask::setSetPoint] Wrong size of the vectors: " << m_kp.size()
                  << " gains, " << jointPosition.size() << " positions, " << jointVelocity.size()
                  << " velocities." << std::endl;
        return false;
    }
    if (!allFinite(jointPosition, jointPosition.size()) || !allFinite(jointVelocity, jointVelocity.size()))
    {
        std::cerr << "[JointTrackingTask::setSetPoint] The set point is not finite." << std::endl;
        return false;
    }
    m_position = jointPosition;
    m_velocity = jointVelocity;
    m_hasSetPoint = true;
    return true;
}

bool JointLimitsTask::initialize(std::weak_ptr<IParametersHandler> handlerWeak)
{
    constexpr const char* where = "[JointLimitsTask::initialize] ";
    m_isInitialized = false;
    auto handler = handlerWeak.lock();
    if (handler == nullptr)
    {
        std::cerr << where << "The parameters handler no longer exists." << std::endl;
        return false;
    }
    std::vector<double> klim, lower, upper, velocity;
    double samplingTime = 0.0;
    bool useModel = false;
    if (!handler->getParameter("klim", klim) || klim.empty())
    {
        std::cerr << where << "The parameter klim is missing." << std::endl;
        return false;
    }
    for (const double k : klim)
        if (!(k > 0.0 && k <= 1.0))
        {
            std::cerr << where << "The gains klim must be in (0, 1]." << std::endl;
            return false;
        }
    if (!handler->getParameter("sampling_time", samplingTime) || !std::isfinite(samplingTime) || samplingTime <= 0.0)
    {
        std::cerr << where << "The parameter sampling_time is missing or not a positive number." << std::endl;
        return false;
    }
    if (!handler->getParameter("use_model_limits", useModel))
    {
        std::cerr << where << "The parameter use_model_limits is missing." << std::endl;
        return false;
    }
    if (!useModel)
    {
        if (!handler->getParameter("lower_limits", lower) || !handler->getParameter("upper_limits", upper))
        {
            std::cerr << where << "The parameters lower_limits and upper_limits are required without "
                                  "use_model_limits."
                      << std::endl;
            return false;
        }
        if (lower.size() != klim.size() || upper.size() != klim.size())
        {
            std::cerr << where << "Wrong size of the vectors: " << klim.size() << " gains, " << lower.size()
                      << " lower and " << upper.size() << " upper limits." << std::endl;
            return false;
        }
        for (std::size_t j = 0; j < klim.size(); ++j)
            if (!(lower[j] <= upper[j]) || lower[j] == HUGE_VAL || upper[j] == -HUGE_VAL)
            {
                std::cerr << where << "Every lower limit must be at most its upper limit." << std::endl;
                return false;
            }
    }
    if (handler->getParameter("velocity_limits", velocity))
    {
        if (velocity.size() != klim.size())
        {
            std::cerr << where << "The velocity_limits must have one entry per joint." << std::endl;
            return false;
        }
        for (const double v : velocity)
            if (!(v > 0.0))
            {
                std::cerr << where << "The velocity_limits must be positive." << std::endl;
                return false;
            }
    }
    m_klim = klim;
    m_lower = lower;
    m_upper = upper;
    m_velocity = velocity;
    m_samplingTime = samplingTime;
    m_useModelLimits = useModel;
    m_isInitialized = true;
    return true;
}
