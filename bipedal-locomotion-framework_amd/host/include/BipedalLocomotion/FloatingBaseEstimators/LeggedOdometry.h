/**
 * @file LeggedOdometry.h
 * Upstream's Estimators::LeggedOdometry (absent from the reference snapshot; include/blf/blf_c.h
 * section 13 defines it here): the floating base pose and twist from the joint kinematics and a
 * frame held fixed in the world, the fixed frame following the contact states.  Every advance() is
 * one blf_legged_odometry_advance with one robot and one step on the calling thread's handle.
 *
 * Differences a user can notice: the model is a blf::RobotModel set with
 * setRobotModel() (no iDynTree KinDynComputations); every frame of the model is a contact slot, named
 * by setRobotModel's frameNames (or "0", "1", ... without them), at most BLF_ODOM_MAX_CONTACTS;
 * contacts are detected outside (a SchmittTriggerDetector, say) and given with setContactStatus(),
 * which writes the kernel's trigger state directly: the kernel's own triggers are then fed a
 * non-finite force, which section 13 defines as "no change", so detection is bypassed and the
 * switching rule is the section's (the contact on with the latest switch time, no "lastActive"
 * pattern); the world starts at the initial fixed frame unless resetEstimator() places it; rotations
 * are composed and never re-orthonormalised; no IMU and no base-link-IMU transform.
 */
#ifndef BLF_BIPEDAL_LOCOMOTION_FLOATING_BASE_ESTIMATORS_LEGGED_ODOMETRY_H
#define BLF_BIPEDAL_LOCOMOTION_FLOATING_BASE_ESTIMATORS_LEGGED_ODOMETRY_H

#include <memory>
#include <string>
#include <vector>

#include <BipedalLocomotion/ParametersHandler/IParametersHandler.h>
#include <blf/device.h>
#include <blf/robot_model.h>
#include <blf/spatial.h>

namespace BipedalLocomotion
{
namespace Estimators
{

struct LeggedOdometryOutput
{
    blf::Transform basePose;
    blf::Twist baseTwist{{0.0, 0.0, 0.0, 0.0, 0.0, 0.0}};   /**< mixed: (linear, angular) */
};

class LeggedOdometry
{
public:
    /** Reads "initial_fixed_frame" (a frame name).  False if initialised before, the handler is
     * expired or the key is missing. */
    bool initialize(std::weak_ptr<ParametersHandler::IParametersHandler> handlerWeak);

    /** The robot, as FloatingBaseDynamicalSystem::setRobotModel takes it (fixed joints merged);
     * frameNames names the model's frames.  False for a corrupted model, no frame or more than
     * BLF_ODOM_MAX_CONTACTS, a wrong number of names, an initial_fixed_frame that is none of
     * them, or before initialize().  Needs a device. */
    bool setRobotModel(const blf::RobotModel& model, const std::vector<std::string>& frameNames = {});

    /** Places the world: the current fixed frame is held at world_H_fixed from now on. */
    bool resetEstimator(const blf::Transform& world_H_fixed);

    bool setKinematics(const std::vector<double>& jointPositions, const std::vector<double>& jointVelocities);

    /** An externally detected contact: its state and the time it last changed. */
    bool setContactStatus(const std::string& name, bool contactStatus, double switchTime, double timeNow);

    /** Holds another frame fixed from now on, at the world pose the current estimate gives it
     * (blf_fb_frame_state at the last output; needs one advance()). */
    bool changeFixedFrame(const std::string& name);

    bool advance();

    const LeggedOdometryOutput& getOutput() const { return m_output; }
    /** The model's frame index of the fixed frame; -1 before setRobotModel(). */
    int getFixedFrameIdx() const { return m_fixed; }
    /** The world pose at which the fixed frame is held. */
    const blf::Transform& getFixedFramePose() const { return m_fixedPose; }

private:
    enum class State
    {
        NotInitialized,
        Initialized,   // the parameters are read
        Ready,         // and the model is set
        Running
    };
    State m_state{State::NotInitialized};
    std::string m_initialFixedFrame;
    std::vector<std::string> m_names;
    blf::DeviceRobotModel m_model;
    std::vector<double> m_q, m_dq;
    bool m_hasKinematics{false};
    std::vector<int32_t> m_trigState;   // [K]
    std::vector<double> m_trigTimers;   // [K][2]
    double m_time{0.0};
    int m_fixed{-1};
    blf::Transform m_fixedPose;
    LeggedOdometryOutput m_output;

    blf::DeviceBuffer<int32_t> m_dInts;
    blf::DeviceBuffer<double> m_dData;

    int slot(const std::string& name) const;
};

} // namespace Estimators
} // namespace BipedalLocomotion

#endif
