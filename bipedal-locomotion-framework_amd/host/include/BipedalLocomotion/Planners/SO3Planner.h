/**
 * @file SO3Planner.h
 * Minimum-jerk trajectory between two rotations, in the inertial frame: R(t) = Exp(s(t) phi) R0
 * with phi = Log(R1 R0^T) (include/blf/blf_c.h section 11).  The class is absent from the reference
 * snapshot; upstream's Planners library added it later with this interface (setRotations /
 * evaluatePoint).  Every evaluatePoint() is one blf_so3_eval on the calling thread's handle.
 *
 * Differences from upstream a user can notice: rotations are row-major blf::Matrix3 and the
 * velocity / acceleration blf::Vector3 (manif and Eigen are not dependencies); only the inertial
 * (left-trivialised) representation is provided.
 */
#ifndef BLF_BIPEDAL_LOCOMOTION_PLANNERS_SO3_PLANNER_H
#define BLF_BIPEDAL_LOCOMOTION_PLANNERS_SO3_PLANNER_H

#include <vector>

#include <blf/device.h>
#include <blf/spatial.h>

namespace BipedalLocomotion
{
namespace Planners
{

class SO3Planner
{
public:
    /** The boundary rotations and the duration [s]; false unless the duration is positive. */
    bool setRotations(const blf::Matrix3& initialRotation, const blf::Matrix3& finalRotation,
                      double duration);

    /**
     * The rotation, the angular velocity and the angular acceleration (world frame) at `time`.
     * False before setRotations(), for a time outside [0, duration], or without a device.
     */
    bool evaluatePoint(double time, blf::Matrix3& rotation, blf::Vector3& velocity,
                       blf::Vector3& acceleration);

private:
    blf::Matrix3 m_initialRotation{};
    blf::Matrix3 m_finalRotation{};
    double m_T{0.0};
    bool m_areRotationsSet{false};

    std::vector<double> m_staging;        // host image of m_device
    blf::DeviceBuffer<double> m_device;   // R0 9 | R1 9 | T | t | rot 9 | omega 3 | alpha 3
};

} // namespace Planners
} // namespace BipedalLocomotion

#endif // BLF_BIPEDAL_LOCOMOTION_PLANNERS_SO3_PLANNER_H
