/**
 * @file SwingFootPlanner.cpp
 * Parameter handling and return values in the library's convention; the trajectory itself is one
 * blf_swing_foot_eval (one list, every sample) per setContactList().
 */
#include <algorithm>
#include <cmath>
#include <iostream>

#include <BipedalLocomotion/Planners/SwingFootPlanner.h>

using namespace BipedalLocomotion::Planners;
using namespace BipedalLocomotion::ParametersHandler;

bool SwingFootPlanner::initialize(std::weak_ptr<IParametersHandler> handlerWeak)
{
    auto handler = handlerWeak.lock();
    if (handler == nullptr)
    {
        std::cerr << "[SwingFootPlanner::initialize] The parameters handler no longer exists."
                  << std::endl;
        return false;
    }

    double dT = 0.0;
    if (!handler->getParameter("sampling_time", dT))
    {
        std::cerr << "[SwingFootPlanner::initialize] The parameter sampling_time is missing."
                  << std::endl;
        return false;
    }
    if (!(dT > 0.0) || !std::isfinite(dT))
    {
        std::cerr << "[SwingFootPlanner::initialize] The sampling_time must be a strictly positive "
                     "number."
                  << std::endl;
        return false;
    }

    blf_swing_foot_params params{};
    if (!handler->getParameter("step_height", params.step_height))
    {
        std::cerr << "[SwingFootPlanner::initialize] The parameter step_height is missing."
                  << std::endl;
        return false;
    }
    if (!(params.step_height >= 0.0) || !std::isfinite(params.step_height))
    {
        std::cerr << "[SwingFootPlanner::initialize] The step_height must be a non-negative number."
                  << std::endl;
        return false;
    }

    if (!handler->getParameter("foot_apex_time", params.apex_ratio))
    {
        std::cerr << "[SwingFootPlanner::initialize] The parameter foot_apex_time is missing."
                  << std::endl;
        return false;
    }
    if (!(params.apex_ratio > 0.0 && params.apex_ratio < 1.0))
    {
        std::cerr << "[SwingFootPlanner::initialize] The foot_apex_time is a fraction of the swing "
                     "duration: it must be strictly between 0 and 1."
                  << std::endl;
        return false;
    }

    // optional, as upstream: a foot that lands with no vertical velocity or acceleration
    if (!handler->getParameter("foot_landing_velocity", params.landing_velocity))
        params.landing_velocity = 0.0;
    if (!handler->getParameter("foot_landing_acceleration", params.landing_acceleration))
        params.landing_acceleration = 0.0;
    if (!std::isfinite(params.landing_velocity) || !std::isfinite(params.landing_acceleration))
    {
        std::cerr << "[SwingFootPlanner::initialize] The foot_landing_velocity and the "
                     "foot_landing_acceleration must be finite."
                  << std::endl;
        return false;
    }

    m_dT = dT;
    m_params = params;
    m_isInitialized = true;
    m_numSamples = 0;
    return true;
}

bool SwingFootPlanner::setContactList(const ContactList& contactList)
{
    if (!m_isInitialized)
    {
        std::cerr << "[SwingFootPlanner::setContactList] The planner is not initialized: call "
                     "initialize() first."
                  << std::endl;
        return false;
    }
    const std::size_t n = contactList.size();
    if (n == 0)
    {
        std::cerr << "[SwingFootPlanner::setContactList] The contact list is empty." << std::endl;
        return false;
    }
    if (n > BLF_SWING_MAX_CONTACTS)
    {
        std::cerr << "[SwingFootPlanner::setContactList] The contact list has " << n
                  << " contacts, at most " << BLF_SWING_MAX_CONTACTS << " are supported."
                  << std::endl;
        return false;
    }
    const double tFirst = contactList.firstContact()->activationTime;
    const double tLast = contactList.lastContact()->activationTime;
    const double count = std::floor((tLast - tFirst) / m_dT);
    if (!(count >= 0.0 && count < 1.0e7))
    {
        std::cerr << "[SwingFootPlanner::setContactList] The list spans too many samples."
                  << std::endl;
        return false;
    }
    // the samples t_k = t_first + k dT that are not past the last contact's activation
    std::size_t K = static_cast<std::size_t>(count) + 2;
    while (K > 1 && tFirst + static_cast<double>(K - 1) * m_dT > tLast) --K;

    blf_handle* h = blf::threadHandle();
    if (h == nullptr)
    {
        std::cerr << "[SwingFootPlanner::setContactList] No device." << std::endl;
        return false;
    }

    const std::size_t oTime = n * 12, oTq = oTime + n * 2, oPose = oTq + K, oTwist = oPose + K * 12,
                      oAccel = oTwist + K * 6, total = oAccel + K * 6;
    m_staging.assign(total, 0.0);
    std::size_t c = 0;
    for (const Contact& contact : contactList)
    {
        const auto packed = contact.pose.packed();
        std::copy(packed.begin(), packed.end(), m_staging.begin() + c * 12);
        m_staging[oTime + 2 * c] = contact.activationTime;
        m_staging[oTime + 2 * c + 1] = contact.deactivationTime;
        ++c;
    }
    for (std::size_t k = 0; k < K; ++k) m_staging[oTq + k] = tFirst + static_cast<double>(k) * m_dT;
    std::vector<int32_t> ints(1 + K, 0);
    ints[0] = static_cast<int32_t>(n);
    if (!m_device.upload(m_staging) || !m_deviceInt.upload(ints)) return false;

    blf_swing_foot_params params = m_params;
    params.max_contacts = static_cast<int32_t>(n);
    params.reserved = 0;
    double* d = m_device.data();
    int32_t* di = m_deviceInt.data();
    if (!blf::report(blf_swing_foot_eval(h, &params, d, d + oTime, di, 1, d + oTq,
                                         static_cast<int32_t>(K), d + oPose, d + oTwist, d + oAccel,
                                         nullptr, di + 1, nullptr),
                     "SwingFootPlanner::setContactList"))
        return false;
    if (!m_device.download(m_staging.data(), total) || !m_deviceInt.download(ints.data(), 1 + K))
        return false;

    m_contactList = contactList;
    m_samples.swap(m_staging);
    m_inContact.assign(ints.begin() + 1, ints.end());
    m_oTq = oTq;
    m_oPose = oPose;
    m_oTwist = oTwist;
    m_oAccel = oAccel;
    m_numSamples = K;
    m_index = 0;
    loadSample(0);
    return true;
}

void SwingFootPlanner::loadSample(std::size_t k)
{
    const double* pose = m_samples.data() + m_oPose + k * 12;
    std::copy(pose, pose + 3, m_state.transform.position.begin());
    std::copy(pose + 3, pose + 12, m_state.transform.rotation.begin());
    const double* twist = m_samples.data() + m_oTwist + k * 6;
    std::copy(twist, twist + 6, m_state.mixedVelocity.begin());
    const double* accel = m_samples.data() + m_oAccel + k * 6;
    std::copy(accel, accel + 6, m_state.mixedAcceleration.begin());
    m_state.isInContact = m_inContact[k] != 0;
    m_state.time = m_samples[m_oTq + k];
}

const SwingFootPlannerState& SwingFootPlanner::get() const
{
    return m_state;
}

bool SwingFootPlanner::isValid() const
{
    return m_numSamples > 0;
}

bool SwingFootPlanner::advance()
{
    if (!isValid())
    {
        std::cerr << "[SwingFootPlanner::advance] No contact list: call setContactList() first."
                  << std::endl;
        return false;
    }
    if (m_index + 1 >= m_numSamples)
    {
        std::cerr << "[SwingFootPlanner::advance] The trajectory ends at the last contact's "
                     "activation time."
                  << std::endl;
        return false;
    }
    ++m_index;
    loadSample(m_index);
    return true;
}
