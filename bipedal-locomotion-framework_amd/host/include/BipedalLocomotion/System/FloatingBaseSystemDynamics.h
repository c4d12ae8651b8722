/**
 * @file FloatingBaseSystemDynamics.h
 * Drop-in for src/System/include/BipedalLocomotion/System/FloatingBaseSystemDynamics.h:30-157
 * (src/System/src/FloatingBaseSystemDynamics.cpp):
 *   state      (base velocity (mixed), joint velocities, base position, base orientation,
 *               joint positions)
 *   input      (joint torques, contact wrenches)
 *   derivative (base acceleration, joint accelerations, base linear velocity, base rotation rate,
 *               joint velocities)
 * The reference takes M, h and the frame Jacobians from iDynTree KinDynComputations, set with
 * setKinDyn(); this build has no iDynTree, so the robot is given as a kinematic tree with
 * setRobotModel() (blf::RobotModel, the layout of blf/robot.py) and the rigid-body terms are
 * computed on the device (blf_fbd_dynamics / blf_fbd_euler_integrate, include/blf/blf_c.h).
 * Contacts may hold any ContactModel.  A ContinuousContactModel is evaluated in the kernel
 * (BLF_CONTACT_CONTINUOUS); any other model is set to the frame state the device computes
 * (blf_fb_frame_state) and its getContactWrench() is passed to the kernel (BLF_CONTACT_WRENCH):
 * forwardEulerIntegrate() then launches one Euler step at a time, so that the wrench is taken at
 * every step's start state as in the reference.  dynamics() leaves every contact model in its
 * frame's state (the reference's setState side effect, FloatingBaseSystemDynamics.cpp:225-226);
 * the one-launch forwardEulerIntegrate() of ContinuousContactModel-only contacts does not.
 */
#ifndef BLF_BIPEDAL_LOCOMOTION_SYSTEM_FLOATING_BASE_SYSTEM_DYNAMICS_H
#define BLF_BIPEDAL_LOCOMOTION_SYSTEM_FLOATING_BASE_SYSTEM_DYNAMICS_H

#include <tuple>
#include <vector>

#include <BipedalLocomotion/System/ContactWrench.h>
#include <BipedalLocomotion/System/DynamicalSystem.h>
#include <blf/dense.h>
#include <blf/device.h>
#include <blf/robot_model.h>
#include <blf/spatial.h>

namespace BipedalLocomotion
{
namespace System
{

class FloatingBaseDynamicalSystem
    : public DynamicalSystem<
          std::tuple<blf::Vector6, blf::VectorXd, blf::Vector3, blf::Matrix3, blf::VectorXd>,
          std::tuple<blf::Vector6, blf::VectorXd, blf::Vector3, blf::Matrix3, blf::VectorXd>,
          std::tuple<blf::VectorXd, std::vector<ContactWrench>>>
{
    static constexpr std::size_t m_baseDoFs = 6;
    std::size_t m_actuatedDoFs{0};
    double m_rho{0.01};
    blf::Vector3 m_gravity{{0.0, 0.0, -9.81}};
    bool m_useMassMatrixRegularizationTerm{false};
    blf::DeviceRobotModel m_model;
    blf::DeviceBuffer<int32_t> m_dContactFrame, m_dContactLaw;
    blf::DeviceBuffer<double> m_dReg, m_dState, m_dTau, m_dContactParams, m_dNullPose, m_dOut;
    blf::DeviceBuffer<double> m_dContactWrench, m_dFrameOut;
    blf::DeviceBuffer<double> m_dIdIn, m_dIdOut;   // inverseDynamics: joint accelerations | torques, base acceleration
    blf::DeviceBuffer<int32_t> m_dIdStatus;
    std::vector<std::shared_ptr<ContactModels::ContactModel>> m_contactModels;
    bool m_hostContacts{false};   /**< a contact model the kernel cannot evaluate */

    bool prepare(const char* where, blf_fb_model& model, blf_fb_state& state,
                 blf_fb_contacts& contacts);
    bool updateContactModels(const char* where, const blf_fb_model& model,
                             const blf_fb_state& state, bool wrenches);

public:
    bool initalize(std::weak_ptr<ParametersHandler::IParametersHandler> handler) final;
    void setGravityVector(const blf::Vector3& gravity) { m_gravity = gravity; }
    /** Replaces setKinDyn(): the robot model whose rigid-body terms the device computes.  False,
     *  before any device work and with blf::describe's line, for a model blf::prepareRobotModel
     *  refuses (blf/robot_model.h); the model set before stays. */
    bool setRobotModel(const blf::RobotModel& model);
    bool setMassMatrixRegularization(const blf::MatrixXd& matrix);
    bool dynamics(const double& time, StateDerivativeType& stateDerivative) final;

    /**
     * Inverse dynamics with the base free (blf_fb_inverse_dynamics, free-base mode) at the current
     * state, with the contact wrenches of the control input (prepared and updated as dynamics()
     * does; the control input's joint torques are not used): the joint torques that produce
     * jointAcceleration and the base acceleration (mixed: linear, angular) that goes with them.
     * Setting those torques as the control input, dynamics() returns jointAcceleration and
     * baseAcceleration.  The mass-matrix regularization does not enter.
     * @return false, with a line on std::cerr, if no model is set, a size is wrong or the device
     * reports a failure of this robot (a non-finite input, a non-positive inertia pivot).
     */
    bool inverseDynamics(const blf::VectorXd& jointAcceleration, blf::Vector6& baseAcceleration,
                         blf::VectorXd& jointTorques);

    /** Device hook used by ForwardEuler<FloatingBaseDynamicalSystem>. */
    bool forwardEulerIntegrate(double initialTime, double finalTime, double dT);
};

} // namespace System
} // namespace BipedalLocomotion

#endif
