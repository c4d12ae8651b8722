/**
 * @file SchmittTriggerDetector.cpp
 * Parameter handling and state machine of the adapter; the trigger step itself runs on the device
 * through blf_schmitt_trigger_advance (one robot, one sample per advance()).
 */
#include <algorithm>
#include <cmath>
#include <iostream>
#include <limits>

#include <BipedalLocomotion/ContactDetectors/SchmittTriggerDetector.h>

using namespace BipedalLocomotion::Contacts;
using namespace BipedalLocomotion::ParametersHandler;

bool SchmittTriggerDetector::initialize(std::weak_ptr<IParametersHandler> handlerWeak)
{
    const char* where = "[SchmittTriggerDetector::initialize] ";
    if (m_initialized)
    {
        std::cerr << where << "This detector is initialized already." << std::endl;
        return false;
    }
    auto handler = handlerWeak.lock();
    if (handler == nullptr)
    {
        std::cerr << where << "The parameters handler no longer exists." << std::endl;
        return false;
    }
    std::vector<std::string> names;
    if (!handler->getParameter("contacts", names))
    {
        std::cerr << where << "The parameter contacts is missing." << std::endl;
        return false;
    }
    const char* keys[4] = {"contact_make_thresholds", "contact_break_thresholds", "contact_make_switch_times",
                           "contact_break_switch_times"};
    std::vector<double> values[4];
    for (int i = 0; i < 4; ++i)
    {
        if (!handler->getParameter(keys[i], values[i]))
        {
            std::cerr << where << "The parameter " << keys[i] << " is missing." << std::endl;
            return false;
        }
        if (values[i].size() != names.size())
        {
            std::cerr << where << keys[i] << " has " << values[i].size() << " elements, contacts has "
                      << names.size() << "." << std::endl;
            return false;
        }
    }
    const std::size_t K = names.size();
    if (K < 1 || K > BLF_ODOM_MAX_CONTACTS)
    {
        std::cerr << where << K << " contacts: the detector supports 1 to " << BLF_ODOM_MAX_CONTACTS << "."
                  << std::endl;
        return false;
    }
    for (std::size_t c = 0; c < K; ++c)
    {
        if (std::count(names.begin(), names.end(), names[c]) != 1)
        {
            std::cerr << where << "The contact " << names[c] << " is listed twice." << std::endl;
            return false;
        }
        const double on = values[0][c], off = values[1][c], ton = values[2][c], toff = values[3][c];
        if (!(std::isfinite(on) && std::isfinite(off) && std::isfinite(ton) && std::isfinite(toff)) || ton < 0.0
            || toff < 0.0 || on < off)
        {
            std::cerr << where << "The contact " << names[c]
                      << " has a threshold or switch time that is not finite, a negative switch time or a make "
                         "threshold below its break threshold."
                      << std::endl;
            return false;
        }
    }
    m_names = names;
    m_params.resize(4 * K);
    for (std::size_t c = 0; c < K; ++c)
        for (int i = 0; i < 4; ++i) m_params[4 * c + i] = values[i][c];
    m_state.assign(K, 0);
    m_timers.assign(2 * K, 0.0);
    m_value.assign(K, 0.0);
    m_time.assign(K, 0.0);
    m_fresh.assign(K, 0);
    for (const auto& n : names) m_output[n] = EstimatedContact{};
    m_initialized = true;
    return true;
}

int SchmittTriggerDetector::slot(const std::string& name) const
{
    const auto it = std::find(m_names.begin(), m_names.end(), name);
    return it == m_names.end() ? -1 : static_cast<int>(it - m_names.begin());
}

bool SchmittTriggerDetector::setTimedTriggerInput(const std::string& name, double time, double force)
{
    const int c = m_initialized ? slot(name) : -1;
    if (c < 0)
    {
        std::cerr << "[SchmittTriggerDetector::setTimedTriggerInput] "
                  << (m_initialized ? "Unknown contact " + name + "." : std::string("Call initialize() first."))
                  << std::endl;
        return false;
    }
    m_time[c] = time;
    m_value[c] = force;
    m_fresh[c] = 1;
    return true;
}

bool SchmittTriggerDetector::resetContact(const std::string& name, bool state, double time)
{
    const int c = m_initialized ? slot(name) : -1;
    if (c < 0)
    {
        std::cerr << "[SchmittTriggerDetector::resetContact] "
                  << (m_initialized ? "Unknown contact " + name + "." : std::string("Call initialize() first."))
                  << std::endl;
        return false;
    }
    m_state[c] = state ? 1 : 0;
    m_timers[2 * c] = m_timers[2 * c + 1] = time;
    m_output[name] = EstimatedContact{state, time, time};
    return true;
}

bool SchmittTriggerDetector::advance()
{
    const char* where = "[SchmittTriggerDetector::advance] ";
    if (!m_initialized)
    {
        std::cerr << where << "The detector is not initialized: call initialize() first." << std::endl;
        return false;
    }
    const std::size_t K = m_names.size();
    bool any = false;
    double time = 0.0;
    for (std::size_t c = 0; c < K; ++c)
    {
        if (!m_fresh[c]) continue;
        if (any && m_time[c] != time)
        {
            std::cerr << where << "The inputs of one advance() must carry the same time (" << time << " and "
                      << m_time[c] << " given)." << std::endl;
            return false;
        }
        any = true;
        time = m_time[c];
    }
    if (!any)
    {
        std::cerr << where << "No input: call setTimedTriggerInput() first." << std::endl;
        return false;
    }
    blf_handle* h = blf::threadHandle();
    if (h == nullptr)
    {
        std::cerr << where << "No device." << std::endl;
        return false;
    }
    // one upload (time | value K | timers 2K, and the states), one launch, one download
    m_staging.assign(1 + 3 * K, 0.0);
    m_staging[0] = time;
    for (std::size_t c = 0; c < K; ++c)
        m_staging[1 + c] = m_fresh[c] ? m_value[c] : std::numeric_limits<double>::quiet_NaN();   // no sample: no change
    std::copy(m_timers.begin(), m_timers.end(), m_staging.begin() + 1 + K);
    if (!m_device.upload(m_staging) || !m_deviceState.upload(m_state)) return false;
    double* d = m_device.data();
    if (!blf::report(blf_schmitt_trigger_advance(h, static_cast<int32_t>(K), m_params.data(), 0, d, d + 1, 1,
                                                 m_deviceState.data(), d + 1 + K, nullptr, 1, nullptr),
                     "SchmittTriggerDetector::advance"))
        return false;
    if (!m_device.download(m_staging.data(), m_staging.size()) || !m_deviceState.download(m_state.data(), K))
        return false;
    std::copy(m_staging.begin() + 1 + K, m_staging.end(), m_timers.begin());
    for (std::size_t c = 0; c < K; ++c)
    {
        EstimatedContact& e = m_output[m_names[c]];
        e.isActive = (m_state[c] & 1) != 0;
        e.switchTime = m_timers[2 * c + 1];
        if (m_fresh[c]) e.lastUpdateTime = m_time[c];
        m_fresh[c] = 0;
    }
    return true;
}

bool SchmittTriggerDetector::get(const std::string& name, EstimatedContact& contact) const
{
    const auto it = m_output.find(name);
    if (it == m_output.end())
    {
        std::cerr << "[SchmittTriggerDetector::get] Unknown contact " << name << "." << std::endl;
        return false;
    }
    contact = it->second;
    return true;
}
