/**
 * @file LeggedOdometry.cpp
 * Parameter handling and state machine of the adapter; the estimate itself is one
 * blf_legged_odometry_advance (one robot, one step) per advance().
 */
#include <algorithm>
#include <cmath>
#include <iostream>
#include <limits>

#include <BipedalLocomotion/FloatingBaseEstimators/LeggedOdometry.h>

using namespace BipedalLocomotion::Estimators;
using namespace BipedalLocomotion::ParametersHandler;

namespace
{
// detection is bypassed: no force reaches the kernel's triggers (see setContactStatus), so their
// parameters are never used; they only have to be ones the call accepts
const double kUnusedParams[4] = {1.0, 0.0, 0.0, 0.0};

bool fail(const char* where, const std::string& what)
{
    std::cerr << "[LeggedOdometry::" << where << "] " << what << std::endl;
    return false;
}
} // namespace

bool LeggedOdometry::initialize(std::weak_ptr<IParametersHandler> handlerWeak)
{
    if (m_state != State::NotInitialized) return fail("initialize", "This estimator is initialized already.");
    auto handler = handlerWeak.lock();
    if (handler == nullptr) return fail("initialize", "The parameters handler no longer exists.");
    if (!handler->getParameter("initial_fixed_frame", m_initialFixedFrame))
        return fail("initialize", "The parameter initial_fixed_frame is missing.");
    m_state = State::Initialized;
    return true;
}

int LeggedOdometry::slot(const std::string& name) const
{
    const auto it = std::find(m_names.begin(), m_names.end(), name);
    return it == m_names.end() ? -1 : static_cast<int>(it - m_names.begin());
}

bool LeggedOdometry::setRobotModel(const blf::RobotModel& fullModel, const std::vector<std::string>& frameNames)
{
    const char* where = "setRobotModel";
    if (m_state == State::NotInitialized) return fail(where, "Call initialize() first.");
    if (!fullModel.fixedJoint.empty() && !blf::fixedJointMergeable(fullModel))
        return fail(where, "Corrupted robot model.");
    const blf::RobotModel model = fullModel.fixedJoint.empty() ? fullModel : blf::reduceFixedJoints(fullModel);
    const std::size_t n = static_cast<std::size_t>(model.ndof < 0 ? 0 : model.ndof), F = model.frameLink.size();
    if (model.ndof < 1 || model.ndof > BLF_FBD_MAX_DOFS || model.parent.size() != n || model.jointOrigin.size() != 3 * n
        || model.jointRotation.size() != 9 * n || model.jointAxis.size() != 3 * n || model.linkMass.size() != n + 1
        || model.linkCom.size() != 3 * (n + 1) || model.linkInertia.size() != 9 * (n + 1)
        || model.framePose.size() != 12 * F || (!model.jointType.empty() && model.jointType.size() != n))
        return fail(where, "Corrupted robot model.");
    for (std::size_t j = 0; j < n; ++j)
        if (model.parent[j] < 0 || model.parent[j] > static_cast<int32_t>(j))
            return fail(where, "The joints must be in topological order (parent[j] <= j).");
    for (const int32_t t : model.jointType)
        if (t != BLF_JOINT_REVOLUTE && t != BLF_JOINT_PRISMATIC)
            return fail(where, "Unknown joint type " + std::to_string(t) + ".");
    for (const int32_t l : model.frameLink)
        if (l < 0 || l > model.ndof) return fail(where, "A frame is attached to a link the model does not have.");
    if (F < 1 || F > BLF_ODOM_MAX_CONTACTS)
        return fail(where, std::to_string(F) + " frames: every frame is a contact slot, 1 to "
                               + std::to_string(BLF_ODOM_MAX_CONTACTS) + " are supported.");
    if (!frameNames.empty() && frameNames.size() != F)
        return fail(where, std::to_string(frameNames.size()) + " frame names for " + std::to_string(F) + " frames.");
    std::vector<std::string> names = frameNames;
    for (std::size_t f = 0; names.size() < F; ++f) names.push_back(std::to_string(f));
    const auto it = std::find(names.begin(), names.end(), m_initialFixedFrame);
    if (it == names.end()) return fail(where, "The model has no frame named " + m_initialFixedFrame + ".");
    if (blf::threadHandle() == nullptr) return fail(where, "No device.");
    if (!(m_dParent.upload(model.parent) && m_dOrigin.upload(model.jointOrigin) && m_dRot.upload(model.jointRotation)
          && m_dAxis.upload(model.jointAxis) && m_dMass.upload(model.linkMass) && m_dCom.upload(model.linkCom)
          && m_dInertia.upload(model.linkInertia) && m_dFrameLink.upload(model.frameLink)
          && m_dFramePose.upload(model.framePose) && (model.jointType.empty() || m_dJointType.upload(model.jointType))))
        return fail(where, "The model could not be copied to the device.");
    m_model = model;
    m_names = names;
    m_fixed = static_cast<int>(it - names.begin());
    m_fixedPose = blf::Transform::Identity();   // the world starts at the initial fixed frame
    m_trigState.assign(F, 0);
    m_trigState[m_fixed] = 1;
    m_trigTimers.assign(2 * F, 0.0);
    m_q.assign(n, 0.0);
    m_dq.assign(n, 0.0);
    m_hasKinematics = false;
    m_state = State::Ready;
    return true;
}

bool LeggedOdometry::resetEstimator(const blf::Transform& world_H_fixed)
{
    if (m_state != State::Ready && m_state != State::Running) return fail("resetEstimator", "Call setRobotModel() first.");
    m_fixedPose = world_H_fixed;
    return true;
}

bool LeggedOdometry::setKinematics(const std::vector<double>& q, const std::vector<double>& dq)
{
    if (m_state != State::Ready && m_state != State::Running) return fail("setKinematics", "Call setRobotModel() first.");
    if (q.size() != m_q.size() || dq.size() != m_dq.size())
        return fail("setKinematics", "Wrong size of the vectors: " + std::to_string(m_q.size()) + " joints.");
    m_q = q;
    m_dq = dq;
    m_hasKinematics = true;
    return true;
}

bool LeggedOdometry::setContactStatus(const std::string& name, bool contactStatus, double switchTime, double timeNow)
{
    if (m_state != State::Ready && m_state != State::Running) return fail("setContactStatus", "Call setRobotModel() first.");
    const int c = slot(name);
    if (c < 0) return fail("setContactStatus", "Unknown contact " + name + ".");
    if (!std::isfinite(switchTime) || !std::isfinite(timeNow)) return fail("setContactStatus", "A time is not finite.");
    m_trigState[c] = contactStatus ? 1 : 0;
    m_trigTimers[2 * c] = m_trigTimers[2 * c + 1] = switchTime;
    m_time = timeNow;
    return true;
}

// the blf_fb_model over the device copies
static blf_fb_model deviceModel(const blf::RobotModel& m, const int32_t* parent, const double* origin, const double* rot,
                                const double* axis, const double* mass, const double* com, const double* inertia,
                                const int32_t* frameLink, const double* framePose, const int32_t* jointType)
{
    blf_fb_model d{};
    d.ndof = m.ndof;
    d.nframes = static_cast<int32_t>(m.frameLink.size());
    d.parent = parent;
    d.joint_origin = origin;
    d.joint_rot = rot;
    d.joint_axis = axis;
    d.link_mass = mass;
    d.link_com = com;
    d.link_inertia = inertia;
    d.frame_link = frameLink;
    d.frame_pose = framePose;
    d.gravity[2] = -9.81;
    d.rho = 0.0;
    d.joint_type = m.jointType.empty() ? nullptr : jointType;
    return d;
}

bool LeggedOdometry::advance()
{
    const char* where = "advance";
    if (m_state != State::Ready && m_state != State::Running)
        return fail(where, "The estimator is not ready: call initialize() and setRobotModel() first.");
    if (!m_hasKinematics) return fail(where, "No kinematics: call setKinematics() first.");
    blf_handle* h = blf::threadHandle();
    if (h == nullptr) return fail(where, "No device.");
    const std::size_t n = m_q.size(), K = m_names.size();
    // doubles: time 1 | q n | dq n | force K | timers 2K | fixed_pose 12 | base pos 3, rot 9, vel 6
    const std::size_t oQ = 1, oDq = oQ + n, oF = oDq + n, oT = oF + K, oP = oT + 2 * K, oOut = oP + 12, total = oOut + 18;
    std::vector<double> data(total, 0.0);
    data[0] = m_time;
    std::copy(m_q.begin(), m_q.end(), data.begin() + oQ);
    std::copy(m_dq.begin(), m_dq.end(), data.begin() + oDq);
    for (std::size_t c = 0; c < K; ++c) data[oF + c] = std::numeric_limits<double>::quiet_NaN();   // detection bypassed
    std::copy(m_trigTimers.begin(), m_trigTimers.end(), data.begin() + oT);
    const auto fp = m_fixedPose.packed();
    std::copy(fp.begin(), fp.end(), data.begin() + oP);
    // ints: frames K | trig_state K | fixed_frame 1 | status 1
    std::vector<int32_t> ints(2 * K + 2, 0);
    for (std::size_t c = 0; c < K; ++c) ints[c] = static_cast<int32_t>(c);
    std::copy(m_trigState.begin(), m_trigState.end(), ints.begin() + K);
    ints[2 * K] = m_fixed;
    if (!m_dData.upload(data) || !m_dInts.upload(ints)) return fail(where, "The inputs could not be copied to the device.");
    const blf_fb_model dm = deviceModel(m_model, m_dParent.data(), m_dOrigin.data(), m_dRot.data(), m_dAxis.data(),
                                        m_dMass.data(), m_dCom.data(), m_dInertia.data(), m_dFrameLink.data(),
                                        m_dFramePose.data(), m_dJointType.data());
    double* d = m_dData.data();
    int32_t* i = m_dInts.data();
    if (!blf::report(blf_legged_odometry_advance(h, &dm, static_cast<int32_t>(K), i, kUnusedParams, 1, d, d + oQ, d + oDq,
                                                 d + oF, 1, i + K, d + oT, i + 2 * K, d + oP, d + oOut, d + oOut + 3,
                                                 d + oOut + 12, nullptr, nullptr, i + 2 * K + 1, 1, 0, nullptr),
                     "LeggedOdometry::advance"))
        return false;
    if (!m_dData.download(data.data(), total) || !m_dInts.download(ints.data(), ints.size()))
        return fail(where, "The outputs could not be copied from the device.");
    if (ints[2 * K + 1] != BLF_IK_OK)
        return fail(where, "The kinematics or the fixed frame's pose are not finite; the estimate is unchanged.");
    m_fixed = ints[2 * K];
    for (int k = 0; k < 3; ++k) m_fixedPose.position[k] = data[oP + k];
    for (int k = 0; k < 9; ++k) m_fixedPose.rotation[k] = data[oP + 3 + k];
    for (int k = 0; k < 3; ++k) m_output.basePose.position[k] = data[oOut + k];
    for (int k = 0; k < 9; ++k) m_output.basePose.rotation[k] = data[oOut + 3 + k];
    for (int k = 0; k < 6; ++k) m_output.baseTwist[k] = data[oOut + 12 + k];
    m_state = State::Running;
    return true;
}

bool LeggedOdometry::changeFixedFrame(const std::string& name)
{
    const char* where = "changeFixedFrame";
    if (m_state != State::Running) return fail(where, "No estimate yet: call advance() first.");
    const int c = slot(name);
    if (c < 0) return fail(where, "Unknown frame " + name + ".");
    blf_handle* h = blf::threadHandle();
    if (h == nullptr) return fail(where, "No device.");
    // the frame's world pose at the last estimate: blf_fb_frame_state at (basePose, q)
    const std::size_t n = m_q.size();
    std::vector<double> st(18 + 2 * n + 12, 0.0);   // base vel 6 | joint vel n | base pos 3 | base rot 9 | joint pos n | pose 12
    for (int k = 0; k < 3; ++k) st[6 + n + k] = m_output.basePose.position[k];
    for (int k = 0; k < 9; ++k) st[9 + n + k] = m_output.basePose.rotation[k];
    std::copy(m_q.begin(), m_q.end(), st.begin() + 18 + n);
    std::vector<int32_t> frame(1, c);
    if (!m_dData.upload(st) || !m_dInts.upload(frame)) return fail(where, "The inputs could not be copied to the device.");
    const blf_fb_model dm = deviceModel(m_model, m_dParent.data(), m_dOrigin.data(), m_dRot.data(), m_dAxis.data(),
                                        m_dMass.data(), m_dCom.data(), m_dInertia.data(), m_dFrameLink.data(),
                                        m_dFramePose.data(), m_dJointType.data());
    double* d = m_dData.data();
    blf_fb_state s{};
    s.base_vel = d;
    s.joint_vel = d + 6;
    s.base_pos = d + 6 + n;
    s.base_rot = d + 9 + n;
    s.joint_pos = d + 18 + n;
    if (!blf::report(blf_fb_frame_state(h, &dm, &s, 1, m_dInts.data(), 1, d + 18 + 2 * n, nullptr, nullptr),
                     "LeggedOdometry::changeFixedFrame"))
        return false;
    if (!m_dData.download(st.data(), st.size())) return fail(where, "The pose could not be copied from the device.");
    for (int k = 0; k < 3; ++k) m_fixedPose.position[k] = st[18 + 2 * n + k];
    for (int k = 0; k < 9; ++k) m_fixedPose.rotation[k] = st[18 + 2 * n + 3 + k];
    m_fixed = c;
    return true;
}
