/**
 * @file SO3Planner.cpp
 * One blf_so3_eval (one trajectory, one query) per evaluatePoint().
 */
#include <algorithm>
#include <cmath>
#include <iostream>

#include <BipedalLocomotion/Planners/SO3Planner.h>

using namespace BipedalLocomotion::Planners;

bool SO3Planner::setRotations(const blf::Matrix3& initialRotation,
                              const blf::Matrix3& finalRotation, double duration)
{
    if (!(duration > 0.0) || !std::isfinite(duration))
    {
        std::cerr << "[SO3Planner::setRotations] The trajectory duration must be a strictly "
                     "positive number."
                  << std::endl;
        return false;
    }
    m_initialRotation = initialRotation;
    m_finalRotation = finalRotation;
    m_T = duration;
    m_areRotationsSet = true;
    return true;
}

bool SO3Planner::evaluatePoint(double time, blf::Matrix3& rotation, blf::Vector3& velocity,
                               blf::Vector3& acceleration)
{
    if (!m_areRotationsSet)
    {
        std::cerr << "[SO3Planner::evaluatePoint] Please set the rotations before evaluating a "
                     "point."
                  << std::endl;
        return false;
    }
    if (!(time >= 0.0 && time <= m_T))
    {
        std::cerr << "[SO3Planner::evaluatePoint] The time has to be a real positive number "
                     "between 0 and "
                  << m_T << "." << std::endl;
        return false;
    }
    blf_handle* h = blf::threadHandle();
    if (h == nullptr)
    {
        std::cerr << "[SO3Planner::evaluatePoint] No device." << std::endl;
        return false;
    }
    const std::size_t oR1 = 9, oT = 18, oQ = 19, oRot = 20, oW = 29, oA = 32, total = 35;
    m_staging.assign(total, 0.0);
    std::copy(m_initialRotation.begin(), m_initialRotation.end(), m_staging.begin());
    std::copy(m_finalRotation.begin(), m_finalRotation.end(), m_staging.begin() + oR1);
    m_staging[oT] = m_T;
    m_staging[oQ] = time;
    if (!m_device.upload(m_staging)) return false;
    double* d = m_device.data();
    if (!blf::report(blf_so3_eval(h, d, d + oR1, d + oT, 1, d + oQ, 1, d + oRot, d + oW, d + oA,
                                  nullptr),
                     "SO3Planner::evaluatePoint"))
        return false;
    if (!m_device.download(m_staging.data(), total)) return false;
    std::copy(m_staging.begin() + oRot, m_staging.begin() + oW, rotation.begin());
    std::copy(m_staging.begin() + oW, m_staging.begin() + oA, velocity.begin());
    std::copy(m_staging.begin() + oA, m_staging.end(), acceleration.begin());
    return true;
}
