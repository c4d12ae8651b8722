/**
 * @file SwingFootPlanner.h
 * SE(3) trajectory of one foot over its ContactList: the contact's pose while the foot is in
 * contact, and between two contacts a quintic-spline translation through an apex with a
 * minimum-jerk rotation (include/blf/blf_c.h section 11).  The class is absent from the reference
 * snapshot; upstream's Planners library added it later as an Advanceable over a ContactList with
 * these parameter keys.  setContactList() evaluates every sample of the list in one
 * blf_swing_foot_eval call; advance() walks the samples on the host.
 *
 * Differences from upstream a user can notice: the state holds blf::Transform / blf::Vector6
 * (manif and Eigen are not dependencies); a list holds at most BLF_SWING_MAX_CONTACTS contacts;
 * setting a new list restarts the walk at the new list's first activation time.
 */
#ifndef BLF_BIPEDAL_LOCOMOTION_PLANNERS_SWING_FOOT_PLANNER_H
#define BLF_BIPEDAL_LOCOMOTION_PLANNERS_SWING_FOOT_PLANNER_H

#include <cstddef>
#include <memory>
#include <vector>

#include <BipedalLocomotion/ParametersHandler/IParametersHandler.h>
#include <BipedalLocomotion/Planners/ContactList.h>
#include <BipedalLocomotion/System/Advanceable.h>
#include <blf/device.h>
#include <blf/spatial.h>

namespace BipedalLocomotion
{
namespace Planners
{

struct SwingFootPlannerState
{
    blf::Transform transform;           /**< world_T_foot */
    blf::Vector6 mixedVelocity{};       /**< (linear, angular), mixed representation */
    blf::Vector6 mixedAcceleration{};   /**< (linear, angular), mixed representation */
    bool isInContact{true};
    double time{0.0};                   /**< the sample's time [s] */
};

class SwingFootPlanner : public System::Advanceable<SwingFootPlannerState>
{
public:
    /**
     * Read "sampling_time" (> 0), "step_height" (>= 0), "foot_apex_time" (the apex time as a
     * fraction of the swing, in (0, 1)) and, optionally (default 0), "foot_landing_velocity" and
     * "foot_landing_acceleration".  False if the handler is expired, a required key is missing or
     * a value is out of range.
     */
    bool initialize(std::weak_ptr<ParametersHandler::IParametersHandler> handler);

    /**
     * Set the contacts and evaluate the samples t_k = t_first + k * sampling_time, from the first
     * contact's activation to the last contact's activation, on the device.  get() then holds
     * sample 0.  False before initialize(), for an empty or too long list, or without a device.
     */
    bool setContactList(const ContactList& contactList);

    const SwingFootPlannerState& get() const final;
    bool isValid() const final;

    /** Move to the next sample; false (state unchanged) past the last contact's activation. */
    bool advance() final;

private:
    void loadSample(std::size_t k);

    bool m_isInitialized{false};
    double m_dT{0.0};
    blf_swing_foot_params m_params{};
    ContactList m_contactList;

    std::size_t m_index{0};
    std::size_t m_numSamples{0};
    std::vector<double> m_samples;        // host image of m_device after the evaluation
    std::size_t m_oTq{0}, m_oPose{0}, m_oTwist{0}, m_oAccel{0};   // offsets into it
    std::vector<int32_t> m_inContact;
    SwingFootPlannerState m_state;

    std::vector<double> m_staging;
    blf::DeviceBuffer<double> m_device;   // pose n 12 | time n 2 | tq K | pose K 12 | twist K 6 | accel K 6
    blf::DeviceBuffer<int32_t> m_deviceInt;   // ncontacts | in_contact K
};

} // namespace Planners
} // namespace BipedalLocomotion

#endif // BLF_BIPEDAL_LOCOMOTION_PLANNERS_SWING_FOOT_PLANNER_H
