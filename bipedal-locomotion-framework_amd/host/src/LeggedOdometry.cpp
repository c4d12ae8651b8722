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
const double kGravity[3] = {0.0, 0.0, -9.81};

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
    blf::RobotModel model;
    const blf::ModelDefect defect = blf::prepareRobotModel(fullModel, model);
    if (defect != blf::ModelDefect::None) return fail(where, blf::describe(defect, model));
    const std::size_t n = static_cast<std::size_t>(model.ndof), F = model.frameLink.size();
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
    if (!m_model.set(model)) return fail(where, "The model could not be copied to the device.");
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
    const blf_fb_model dm = m_model.view(kGravity, 0.0);
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
    const std::size_t oPose = blf::fbStateSize(n);
    std::vector<double> st(oPose + 12, 0.0);   // the state, its velocities zero | pose 12
    const blf_fb_state hs = blf::fbStateAt(st.data(), n);
    std::copy(m_output.basePose.position.begin(), m_output.basePose.position.end(), hs.base_pos);
    std::copy(m_output.basePose.rotation.begin(), m_output.basePose.rotation.end(), hs.base_rot);
    std::copy(m_q.begin(), m_q.end(), hs.joint_pos);
    std::vector<int32_t> frame(1, c);
    if (!m_dData.upload(st) || !m_dInts.upload(frame)) return fail(where, "The inputs could not be copied to the device.");
    const blf_fb_model dm = m_model.view(kGravity, 0.0);
    double* d = m_dData.data();
    const blf_fb_state s = blf::fbStateAt(d, n);
    if (!blf::report(blf_fb_frame_state(h, &dm, &s, 1, m_dInts.data(), 1, d + oPose, nullptr, nullptr),
                     "LeggedOdometry::changeFixedFrame"))
        return false;
    if (!m_dData.download(st.data(), st.size())) return fail(where, "The pose could not be copied from the device.");
    for (int k = 0; k < 3; ++k) m_fixedPose.position[k] = st[oPose + k];
    for (int k = 0; k < 9; ++k) m_fixedPose.rotation[k] = st[oPose + 3 + k];
    m_fixed = c;
    return true;
}
