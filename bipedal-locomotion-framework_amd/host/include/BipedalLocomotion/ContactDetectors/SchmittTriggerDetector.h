/**
 * @file SchmittTriggerDetector.h
 * Upstream's Contacts::SchmittTriggerDetector (absent from the reference snapshot; include/blf/blf_c.h
 * section 13 defines it here): one Schmitt trigger per named contact on the contact's normal force,
 * with upstream's method names and parameter keys.  Every advance() is one
 * blf_schmitt_trigger_advance with one robot, the detector's contacts and one sample, on the calling
 * thread's library handle.
 *
 * Differences a user can notice: an advance() has ONE clock: the inputs set since the
 * previous advance() must carry the same time, otherwise advance() returns false; a contact without
 * a new input keeps its state (it is fed a non-finite sample, which section 13 defines as "no change");
 * at most BLF_ODOM_MAX_CONTACTS contacts; EstimatedContact holds the three fields the detector writes.
 */
#ifndef BLF_BIPEDAL_LOCOMOTION_CONTACT_DETECTORS_SCHMITT_TRIGGER_DETECTOR_H
#define BLF_BIPEDAL_LOCOMOTION_CONTACT_DETECTORS_SCHMITT_TRIGGER_DETECTOR_H

#include <map>
#include <memory>
#include <string>
#include <vector>

#include <BipedalLocomotion/ParametersHandler/IParametersHandler.h>
#include <blf/device.h>

namespace BipedalLocomotion
{
namespace Contacts
{

struct EstimatedContact
{
    bool isActive{false};
    double switchTime{0.0};     /**< time of the last change of isActive */
    double lastUpdateTime{0.0}; /**< time of the last sample the contact was given */
};

class SchmittTriggerDetector
{
public:
    /**
     * Reads "contacts" (the names), "contact_make_thresholds", "contact_break_thresholds",
     * "contact_make_switch_times" and "contact_break_switch_times" (one value per contact).  False if
     * the detector was initialised before, the handler is expired, a key is missing, the sizes
     * differ, a name repeats, or a value is one blf_schmitt_trigger_advance refuses (not finite, a
     * negative switch time, a make threshold below its break threshold).
     */
    bool initialize(std::weak_ptr<ParametersHandler::IParametersHandler> handlerWeak);

    /** The sample of one contact for the next advance(); false for an unknown name or before initialize(). */
    bool setTimedTriggerInput(const std::string& name, double time, double force);

    /** One sample of every contact that was given an input; false before initialize(), without any new
     * input, or when the new inputs carry different times. */
    bool advance();

    /** Sets a contact's state directly (upstream's resetContact). */
    bool resetContact(const std::string& name, bool state, double time = 0.0);

    bool get(const std::string& name, EstimatedContact& contact) const;
    const std::map<std::string, EstimatedContact>& getOutput() const { return m_output; }

private:
    std::vector<std::string> m_names;
    std::vector<double> m_params;   // [K][4]
    std::vector<int32_t> m_state;   // [K]
    std::vector<double> m_timers;   // [K][2]
    std::vector<double> m_value, m_time;
    std::vector<uint8_t> m_fresh;
    std::map<std::string, EstimatedContact> m_output;
    bool m_initialized{false};

    std::vector<double> m_staging;
    blf::DeviceBuffer<double> m_device;       // time 1 | value K | timers 2K
    blf::DeviceBuffer<int32_t> m_deviceState; // state K

    int slot(const std::string& name) const;
};

} // namespace Contacts
} // namespace BipedalLocomotion

#endif
