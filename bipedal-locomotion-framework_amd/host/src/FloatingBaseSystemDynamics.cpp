/**
 * @file FloatingBaseSystemDynamics.cpp
 * Checks and messages follow src/System/src/FloatingBaseSystemDynamics.cpp:17-120; the dynamics
 * (:102-251) run on the device through blf_fbd_dynamics / blf_fbd_euler_integrate.
 */
#include <iostream>

#include <BipedalLocomotion/ContactModels/ContinuousContactModel.h>
#include <BipedalLocomotion/System/FloatingBaseSystemDynamics.h>

using namespace BipedalLocomotion::System;
using namespace BipedalLocomotion::ParametersHandler;

bool FloatingBaseDynamicalSystem::initalize(std::weak_ptr<IParametersHandler> handler)
{
    auto ptr = handler.lock();
    if (ptr == nullptr)
    {
        std::cerr << "[FloatingBaseDynamicalSystem::initalize] The parameter handler is expired. "
                     "Please call the function passing a pointer pointing an already allocated "
                     "memory."
                  << std::endl;
        return false;
    }
    if (!ptr->getParameter("rho", m_rho))
    {
        std::cerr << "[FloatingBaseDynamicalSystem::initalize] Unable to load the Baumgarte "
                     "stabilization parameter."
                  << std::endl;
        return false;
    }
    return true;
}

bool FloatingBaseDynamicalSystem::setRobotModel(const blf::RobotModel& fullModel)
{
    blf::RobotModel model;
    const blf::ModelDefect defect = blf::prepareRobotModel(fullModel, model);
    if (defect != blf::ModelDefect::None)
    {
        std::cerr << "[FloatingBaseDynamicalSystem::setRobotModel] " << blf::describe(defect, model)
                  << std::endl;
        return false;
    }
    m_actuatedDoFs = static_cast<std::size_t>(model.ndof);
    return m_model.set(model);
}

bool FloatingBaseDynamicalSystem::setMassMatrixRegularization(const blf::MatrixXd& matrix)
{
    if (!m_model.ok())
    {
        std::cerr << "[FloatingBaseDynamicalSystem::setMassMatrixRegularization] Please call "
                     "'setRobotModel()' before."
                  << std::endl;
        return false;
    }
    const std::size_t rightSize = m_actuatedDoFs + m_baseDoFs;
    if (rightSize != matrix.rows() || matrix.cols() != matrix.rows())
    {
        std::cerr << "[FloatingBaseDynamicalSystem::setMassMatrixRegularization] The size of the "
                     "regularization matrix is not correct. The correct size is: "
                  << rightSize << " x " << rightSize << ". While the input of the function is a "
                  << matrix.rows() << " x " << matrix.cols() << " matrix." << std::endl;
        return false;
    }
    m_useMassMatrixRegularizationTerm = m_dReg.upload(matrix.data(), rightSize * rightSize);
    return m_useMassMatrixRegularizationTerm;
}

bool FloatingBaseDynamicalSystem::prepare(const char* where, blf_fb_model& model,
                                          blf_fb_state& state, blf_fb_contacts& contacts)
{
    if (!m_model.ok())
    {
        std::cerr << "[" << where << "] Please call 'setRobotModel()' before." << std::endl;
        return false;
    }
    const auto& [baseVelocity, jointVelocity, basePosition, baseOrientation, jointPositions] = m_state;
    const auto& [jointTorques, contactWrenches] = m_controlInput;
    const std::size_t n = m_actuatedDoFs;
    if (jointVelocity.size() != n || jointPositions.size() != n || jointTorques.size() != n)
    {
        std::cerr << "[" << where << "] Wrong size of the vectors." << std::endl;
        return false;
    }
    if (contactWrenches.size() > BLF_FBD_MAX_CONTACTS)
    {
        std::cerr << "[" << where << "] At most " << BLF_FBD_MAX_CONTACTS << " contacts." << std::endl;
        return false;
    }
    std::vector<double> st(blf::fbStateSize(n));
    blf::fbStatePack(baseVelocity, jointVelocity, basePosition, baseOrientation, jointPositions, st.data());
    std::vector<int32_t> frames, laws;
    std::vector<double> params, nulls;
    m_contactModels.clear();
    m_hostContacts = false;
    for (const auto& c : contactWrenches)
    {
        auto ptr = c.contactModel().lock();
        if (ptr == nullptr)
        {
            std::cerr << "[" << where << "] The contact model associated to the frame " << c.index()
                      << " has been expired." << std::endl;
            return false;
        }
        if (c.index() < 0 || c.index() >= static_cast<int>(m_model.host().frameLink.size()))
        {
            std::cerr << "[" << where << "] Unknown frame " << c.index() << "." << std::endl;
            return false;
        }
        frames.push_back(c.index());
        // a ContinuousContactModel is evaluated in the kernel; any other model by its own
        // getContactWrench() at the frame state the device computes (BLF_CONTACT_WRENCH)
        auto cm = std::dynamic_pointer_cast<ContactModels::ContinuousContactModel>(ptr);
        if (cm != nullptr)
        {
            laws.push_back(BLF_CONTACT_CONTINUOUS);
            params.insert(params.end(), {cm->length(), cm->width(), cm->springCoeff(), cm->damperCoeff()});
            const auto np = cm->nullForceTransform().packed();
            nulls.insert(nulls.end(), np.begin(), np.end());
        } else
        {
            laws.push_back(BLF_CONTACT_WRENCH);
            m_hostContacts = true;
            params.insert(params.end(), 4, 0.0);
            const auto np = blf::Transform::Identity().packed();
            nulls.insert(nulls.end(), np.begin(), np.end());
        }
        m_contactModels.push_back(ptr);
    }
    if (m_hostContacts
        && (!m_dContactLaw.upload(laws) || !m_dContactWrench.resize(6 * laws.size())))
        return false;
    if (!m_dState.upload(st) || !m_dTau.upload(jointTorques.data(), n)
        || !m_dContactFrame.upload(frames) || !m_dContactParams.upload(params)
        || !m_dNullPose.upload(nulls))
        return false;
    model = m_model.view(m_gravity.data(), m_rho);
    state = blf::fbStateAt(m_dState.data(), n);
    contacts.ncontacts = static_cast<int32_t>(frames.size());
    contacts.frame = m_dContactFrame.data();
    contacts.params = m_dContactParams.data();
    contacts.null_pose = m_dNullPose.data();
    contacts.law = m_hostContacts ? m_dContactLaw.data() : nullptr;
    contacts.wrench = m_hostContacts ? m_dContactWrench.data() : nullptr;
    return true;
}

// The reference's per-contact `contactPtr->setState(getFrameVel, getWorldTransform)` (FloatingBase
// SystemDynamics.cpp:225-226) at the device's frame state; then, when `wrenches` is set, the
// BLF_CONTACT_WRENCH contacts' getContactWrench() uploaded for the next launch.
bool FloatingBaseDynamicalSystem::updateContactModels(const char* where, const blf_fb_model& model,
                                                      const blf_fb_state& state, bool wrenches)
{
    const std::size_t C = m_contactModels.size();
    if (C == 0) return true;
    blf_handle* h = blf::threadHandle();
    if (!m_dFrameOut.resize(18 * C)) return false;
    double* pose = m_dFrameOut.data();
    if (!blf::report(blf_fb_frame_state(h, &model, &state, static_cast<int32_t>(C),
                                        m_dContactFrame.data(), 1, pose, pose + 12 * C, nullptr),
                     where))
        return false;
    std::vector<double> host(18 * C), wrench(6 * C, 0.0);
    if (!m_dFrameOut.download(host.data(), host.size())) return false;
    for (std::size_t c = 0; c < C; ++c)
    {
        blf::Transform T;
        blf::Twist tw;
        for (int i = 0; i < 3; ++i) T.position[i] = host[12 * c + i];
        for (int i = 0; i < 9; ++i) T.rotation[i] = host[12 * c + 3 + i];
        for (int i = 0; i < 6; ++i) tw[i] = host[12 * C + 6 * c + i];
        m_contactModels[c]->setState(tw, T);
        if (wrenches
            && std::dynamic_pointer_cast<ContactModels::ContinuousContactModel>(m_contactModels[c])
                   == nullptr)
        {
            const blf::Wrench& w = m_contactModels[c]->getContactWrench();
            for (int i = 0; i < 6; ++i) wrench[6 * c + i] = w[i];
        }
    }
    return !wrenches || m_dContactWrench.upload(wrench);
}

bool FloatingBaseDynamicalSystem::dynamics(const double& time, StateDerivativeType& stateDerivative)
{
    (void)time;
    const char* where = "FloatingBaseDynamicalSystem::dynamics";
    blf_fb_model model;
    blf_fb_state state;
    blf_fb_contacts contacts;
    blf_handle* h = blf::threadHandle();
    if (h == nullptr || !prepare(where, model, state, contacts)
        || !updateContactModels(where, model, state, m_hostContacts))
        return false;
    const std::size_t n = m_actuatedDoFs;
    if (!m_dOut.resize(blf::fbStateSize(n))) return false;
    const blf_fb_state out = blf::fbStateAt(m_dOut.data(), n);
    if (!blf::report(blf_fbd_dynamics(h, &model, &state, m_dTau.data(), &contacts,
                                      m_useMassMatrixRegularizationTerm ? m_dReg.data() : nullptr,
                                      1, &out, nullptr),
                     where))
        return false;
    std::vector<double> host(blf::fbStateSize(n));
    if (!m_dOut.download(host.data(), host.size())) return false;
    auto& [baseAcceleration, jointAcceleration, baseLinearVelocity, baseRotationRate,
           jointVelocityOutput] = stateDerivative;
    blf::fbStateUnpack(host.data(), n, baseAcceleration, jointAcceleration, baseLinearVelocity,
                       baseRotationRate, jointVelocityOutput);
    return true;
}

bool FloatingBaseDynamicalSystem::inverseDynamics(const blf::VectorXd& jointAcceleration,
                                                  blf::Vector6& baseAcceleration,
                                                  blf::VectorXd& jointTorques)
{
    const char* where = "FloatingBaseDynamicalSystem::inverseDynamics";
    if (!m_model.ok())
    {
        std::cerr << "[" << where << "] Please call 'setRobotModel()' before." << std::endl;
        return false;
    }
    const std::size_t n = m_actuatedDoFs;
    if (jointAcceleration.size() != n)
    {
        std::cerr << "[" << where << "] Wrong size of the joint acceleration: " << jointAcceleration.size()
                  << ", the model has " << n << " joints." << std::endl;
        return false;
    }
    blf_fb_model model;
    blf_fb_state state;
    blf_fb_contacts contacts;
    blf_handle* h = blf::threadHandle();
    if (h == nullptr || !prepare(where, model, state, contacts)
        || !updateContactModels(where, model, state, m_hostContacts))
        return false;
    if (!m_dIdIn.upload(jointAcceleration.data(), n) || !m_dIdOut.resize(n + 6) || !m_dIdStatus.resize(1))
        return false;
    double* o = m_dIdOut.data();
    if (!blf::report(blf_fb_inverse_dynamics(h, &model, &state, m_dIdIn.data(), nullptr, &contacts, 1, o, o + n,
                                             nullptr, m_dIdStatus.data(), 0, nullptr),
                     where))
        return false;
    std::vector<double> host(n + 6);
    int32_t status = 0;
    if (!m_dIdOut.download(host.data(), host.size()) || !m_dIdStatus.download(&status, 1)) return false;
    if (status != BLF_IK_OK)
    {
        std::cerr << "[" << where << "] The device reports "
                  << (status == BLF_IK_BAD_INPUT ? "a non-finite state, acceleration or contact wrench"
                                                 : "a whole-body inertia that is not positive definite")
                  << " (status " << status << ")." << std::endl;
        return false;
    }
    jointTorques.resize(n);
    for (std::size_t i = 0; i < n; ++i) jointTorques[i] = host[i];
    for (int i = 0; i < 6; ++i) baseAcceleration[i] = host[n + i];
    return true;
}

bool FloatingBaseDynamicalSystem::forwardEulerIntegrate(double initialTime, double finalTime,
                                                        double dT)
{
    const char* where = "FixedStepIntegrator::integrate";
    blf_fb_model model;
    blf_fb_state state;
    blf_fb_contacts contacts;
    blf_handle* h = blf::threadHandle();
    if (h == nullptr || !prepare(where, model, state, contacts)) return false;
    const double* reg = m_useMassMatrixRegularizationTerm ? m_dReg.data() : nullptr;
    if (!m_hostContacts)
    {
        // every contact a ContinuousContactModel: the whole integration in one launch
        if (!blf::report(blf_fbd_euler_integrate(h, &model, &state, m_dTau.data(), &contacts, reg,
                                                 1, initialTime, finalTime, dT, nullptr),
                         where))
            return false;
    } else
    {
        // a model the device cannot evaluate: its wrench from the host before every step, as the
        // reference's dynamics() calls getContactWrench() at each step's start state; one launch
        // of one step each (the device's schedule, ForwardEuler.tpp:18-49)
        int32_t iterations = 0;
        double dT_last = 0.0, t_last = 0.0;
        if (!blf::report(blf_step_schedule(initialTime, finalTime, dT, &iterations, &dT_last, &t_last),
                         where))
            return false;
        for (int32_t it = 0; it < iterations; ++it)
        {
            const double step = it + 1 < iterations ? dT : dT_last;
            if (!updateContactModels(where, model, state, true)
                || !blf::report(blf_fbd_euler_integrate(h, &model, &state, m_dTau.data(), &contacts,
                                                        reg, 1, 0.0, step, step, nullptr),
                                where))
                return false;
        }
    }
    const std::size_t n = m_actuatedDoFs;
    std::vector<double> host(blf::fbStateSize(n));
    if (!m_dState.download(host.data(), host.size())) return false;
    auto& [baseVelocity, jointVelocity, basePosition, baseOrientation, jointPositions] = m_state;
    blf::fbStateUnpack(host.data(), n, baseVelocity, jointVelocity, basePosition, baseOrientation,
                       jointPositions);
    return true;
}
