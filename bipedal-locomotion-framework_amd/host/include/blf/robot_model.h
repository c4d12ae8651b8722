/**
 * @file robot_model.h
 * What every adapter over a blf_fb_model shares (FloatingBaseDynamicalSystem, IK::QPInverseKinematics,
 * Estimators::LeggedOdometry): the robot as the caller gives it (RobotModel), the one validation of
 * it (prepareRobotModel), its device copy (DeviceRobotModel) and the layout of the device state
 * (fbStateAt and the pack / unpack pair).
 */
#ifndef BLF_HOST_ROBOT_MODEL_H
#define BLF_HOST_ROBOT_MODEL_H

#include <cstddef>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include <blf/dense.h>
#include <blf/device.h>
#include <blf/spatial.h>

namespace blf
{
/** Kinematic tree of revolute, prismatic (jointType) and fixed (fixedJoint) joints on a floating
 *  base (see blf_fb_model in blf_c.h). */
struct RobotModel
{
    int ndof{0};
    std::vector<int32_t> parent;       /**< [n]        */
    std::vector<double> jointOrigin;   /**< [n][3]     */
    std::vector<double> jointRotation; /**< [n][9]     */
    std::vector<double> jointAxis;     /**< [n][3]     */
    std::vector<double> linkMass;      /**< [n+1]      */
    std::vector<double> linkCom;       /**< [n+1][3]   */
    std::vector<double> linkInertia;   /**< [n+1][9]   */
    std::vector<int32_t> frameLink;    /**< [F]        */
    std::vector<double> framePose;     /**< [F][12]    */
    /** [n] or empty: 1 marks a fixed joint (a URDF "fixed" joint, no DoF). setRobotModel merges
     *  each fixed joint's child link into its parent (reduceFixedJoints), as iDynTree's model has
     *  no DoF for it; the state and torque vectors then cover the remaining joints only. */
    std::vector<uint8_t> fixedJoint;
    /** [n] or empty (every joint revolute): BLF_JOINT_REVOLUTE / BLF_JOINT_PRISMATIC (the child
     *  link slides along the joint axis by q, URDF "prismatic"). */
    std::vector<int32_t> jointType;
    /** [n] or empty (no limits): the joints' position range, -inf / +inf where a side has none, and
     *  their velocity limit (+inf: none).  blf::loadUrdf fills them from <limit>; the IK's
     *  JointLimitsTask reads them with "use_model_limits".  The dynamics do not use them. */
    std::vector<double> jointLower, jointUpper, jointVelocityLimit;
};

/** The model with every joint marked in model.fixedJoint removed and its child link merged into
 *  the parent link (mass, COM, inertia by the parallel-axis theorem; child joints and frames
 *  re-expressed in the parent link's frame at q = 0), deepest first.  The result has an empty
 *  fixedJoint.  Its rigid-body terms equal the full model's with the fixed joints held at
 *  q = 0, q_dot = 0 (blf/robot.py reduce_fixed_joints, tests/test_fb_dynamics.py). */
RobotModel reduceFixedJoints(const RobotModel& model);
/** Whether reduceFixedJoints can merge `model`: consistent array sizes (fixedJoint of ndof
 *  entries), joints in topological order (parent[j] <= j), frames on existing links.  A model that
 *  fails this comes back from reduceFixedJoints unchanged. */
bool fixedJointMergeable(const RobotModel& model);

enum class ModelDefect
{
    None,
    Corrupted,            /**< a wrong array size, ndof out of range, a fixed joint left unmerged */
    NotTopological,       /**< parent[j] outside [0, j] */
    FrameOnUnknownLink,   /**< frameLink outside [0, ndof] */
    UnknownJointType      /**< neither BLF_JOINT_REVOLUTE nor BLF_JOINT_PRISMATIC */
};
/** The text an adapter prints after its "[Class::setRobotModel] " tag; "" for None. */
const char* describe(ModelDefect defect);
/** The same with the offending value of `reduced` where there is one to name (the joint type). */
std::string describe(ModelDefect defect, const RobotModel& reduced);

/**
 * The validation every setRobotModel runs before any device work: `reduced` receives `full` with its
 * fixed joints merged (`full` itself without a fixedJoint mask), and the first defect found is
 * returned.  The order of the checks decides which defect a model with several reports:
 *   with a fixedJoint mask (what the merge reads has to be sound before it runs):
 *     1. the array sizes, fixedJoint.size() == ndof among them              Corrupted
 *     2. the joints' order                                                   NotTopological
 *     3. the frames' links                                                   FrameOnUnknownLink
 *     4. the merge
 *   then on the merged model, or on `full` when there was no mask:
 *     5. ndof in [1, BLF_FBD_MAX_DOFS]; every array size, with jointType, jointLower, jointUpper
 *        and jointVelocityLimit each empty or of ndof entries and jointLower as long as
 *        jointUpper; no fixedJoint left                                      Corrupted
 *     6. the joints' order, the frames' links, the joint types               their defects
 * `reduced` is unspecified after Corrupted, NotTopological and FrameOnUnknownLink.
 */
ModelDefect prepareRobotModel(const RobotModel& full, RobotModel& reduced);

/** A validated, merged model (prepareRobotModel's `reduced`) and its copy in device memory, one
 *  allocation per array. */
class DeviceRobotModel
{
    struct Arrays
    {
        DeviceBuffer<int32_t> parent, frameLink, jointType;
        DeviceBuffer<double> origin, rot, axis, mass, com, inertia, framePose;
    };
    RobotModel m_host;
    Arrays m_d;
    bool m_ok{false};

public:
    DeviceRobotModel() = default;
    DeviceRobotModel(DeviceRobotModel&& o) noexcept
        : m_host(std::move(o.m_host)), m_d(std::move(o.m_d)), m_ok(std::exchange(o.m_ok, false))
    {
    }

    /** Copies `reduced` to the device in place of the model held before; false (and !ok()) if an
     *  allocation or a copy fails. */
    bool set(const RobotModel& reduced);
    /** Whether the last set() succeeded, so that view() points at a complete model. */
    bool ok() const { return m_ok; }
    const RobotModel& host() const { return m_host; }
    /** The C ABI's description of the device copy; joint_type is null when host().jointType is
     *  empty.  Valid until the next set(). */
    blf_fb_model view(const double gravity[3], double rho) const;
};

/** The device state of one robot of n joints:
 *  base vel 6 | joint vel n | base pos 3 | base rot 9 | joint pos n (doubles). */
inline std::size_t fbStateSize(std::size_t n)
{
    return 18 + 2 * n;
}
/** The five parts of the state that starts at s (host or device memory). */
inline blf_fb_state fbStateAt(double* s, std::size_t n)
{
    return blf_fb_state{s, s + 6, s + 6 + n, s + 9 + n, s + 18 + n};
}
/** The tuple (FloatingBaseDynamicalSystem's state, or its derivative) into fbStateSize(n) doubles
 *  at s, n = jointVel.size() = jointPos.size(), and back. */
void fbStatePack(const Vector6& baseVel, const VectorXd& jointVel, const Vector3& basePos,
                 const Matrix3& baseRot, const VectorXd& jointPos, double* s);
void fbStateUnpack(const double* s, std::size_t n, Vector6& baseVel, VectorXd& jointVel,
                   Vector3& basePos, Matrix3& baseRot, VectorXd& jointPos);
} // namespace blf

#endif // BLF_HOST_ROBOT_MODEL_H
