/**
 * @file RobotModel.cpp
 * The fixed-joint merge, the validation of a blf::RobotModel, its device copy and the device state
 * layout behind blf/robot_model.h.
 */
#include <algorithm>

#include <blf/robot_model.h>

namespace blf
{
namespace
{
// the array sizes of a model of n joints; the joint types and the limits each empty or one per joint
bool sizesConsistent(const RobotModel& in, std::size_t n)
{
    return in.parent.size() == n && in.jointOrigin.size() == 3 * n && in.jointRotation.size() == 9 * n
           && in.jointAxis.size() == 3 * n && in.linkMass.size() == n + 1 && in.linkCom.size() == 3 * (n + 1)
           && in.linkInertia.size() == 9 * (n + 1) && in.framePose.size() == 12 * in.frameLink.size()
           && (in.jointType.empty() || in.jointType.size() == n)
           && (in.jointLower.empty() || in.jointLower.size() == n)
           && (in.jointUpper.empty() || in.jointUpper.size() == n)
           && (in.jointVelocityLimit.empty() || in.jointVelocityLimit.size() == n);
}

// a joint's parent link precedes its child (parent[j] <= j); frames sit on links 0..n
ModelDefect orderAndFrames(const RobotModel& in, std::size_t n)
{
    for (std::size_t j = 0; j < n; ++j)
        if (in.parent[j] < 0 || in.parent[j] > static_cast<int32_t>(j)) return ModelDefect::NotTopological;
    for (const int32_t l : in.frameLink)
        if (l < 0 || l > static_cast<int32_t>(n)) return ModelDefect::FrameOnUnknownLink;
    return ModelDefect::None;
}

// what keeps reduceFixedJoints from merging a model with a fixedJoint mask: the merge re-indexes
// joints and links assuming topological order, and moves frames by link index
ModelDefect mergeDefect(const RobotModel& in)
{
    if (in.ndof < 0) return ModelDefect::Corrupted;
    const std::size_t n0 = static_cast<std::size_t>(in.ndof);
    if (in.fixedJoint.size() != n0 || !sizesConsistent(in, n0)) return ModelDefect::Corrupted;
    return orderAndFrames(in, n0);
}
} // namespace

bool fixedJointMergeable(const RobotModel& in)
{
    return mergeDefect(in) == ModelDefect::None;
}

RobotModel reduceFixedJoints(const RobotModel& in)
{
    // an inconsistent model (sizes, order) comes back unchanged, its fixedJoint still set, so the
    // caller's own validation (prepareRobotModel) reports it instead of a merge reading out of bounds
    if (!fixedJointMergeable(in)) return in;
    RobotModel m = in;
    m.fixedJoint.clear();
    const int n0 = in.ndof;
    auto E = [&](int j, int r, int c) { return m.jointRotation[9 * j + 3 * r + c]; };
    // y = E_j x (3-vectors)
    auto rot = [&](int j, const double* x, double* y) {
        for (int r = 0; r < 3; ++r) y[r] = E(j, r, 0) * x[0] + E(j, r, 1) * x[1] + E(j, r, 2) * x[2];
    };
    // C = E_j A (3x3 row-major)
    auto rotm = [&](int j, const double* A, double* C) {
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c)
                C[3 * r + c] = E(j, r, 0) * A[c] + E(j, r, 1) * A[3 + c] + E(j, r, 2) * A[6 + c];
    };
    // I += m S(d), S(d) = |d|^2 1 - d d^T
    auto pax = [](double* I, double mass, const double* d) {
        const double dd = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) I[3 * r + c] += mass * ((r == c ? dd : 0.0) - d[r] * d[c]);
    };
    for (int j = n0 - 1; j >= 0; --j)
    {
        if (!in.fixedJoint[j]) continue;
        const int c = j + 1, P = m.parent[j];
        double cc[3], cn[3], Ic[9], T[9];
        rot(j, &m.linkCom[3 * c], cc);
        for (int a = 0; a < 3; ++a) cc[a] += m.jointOrigin[3 * j + a];   // child COM in P's frame
        const double mP = m.linkMass[P], mc = m.linkMass[c], mt = mP + mc;
        for (int a = 0; a < 3; ++a) cn[a] = mt > 0 ? (mP * m.linkCom[3 * P + a] + mc * cc[a]) / mt : m.linkCom[3 * P + a];
        // E_j I_c E_j^T
        rotm(j, &m.linkInertia[9 * c], T);
        for (int r = 0; r < 3; ++r)
            for (int k = 0; k < 3; ++k) Ic[3 * r + k] = T[3 * r] * E(j, k, 0) + T[3 * r + 1] * E(j, k, 1) + T[3 * r + 2] * E(j, k, 2);
        double dP[3], dc[3];
        for (int a = 0; a < 3; ++a) { dP[a] = m.linkCom[3 * P + a] - cn[a]; dc[a] = cc[a] - cn[a]; }
        double* IP = &m.linkInertia[9 * P];
        pax(IP, mP, dP);
        for (int k = 0; k < 9; ++k) IP[k] += Ic[k];
        pax(IP, mc, dc);
        m.linkMass[P] = mt;
        for (int a = 0; a < 3; ++a) m.linkCom[3 * P + a] = cn[a];
        for (int k = j + 1; k < m.ndof; ++k)   // joints on c move to P
            if (m.parent[k] == c)
            {
                double o[3], R[9];
                rot(j, &m.jointOrigin[3 * k], o);
                rotm(j, &m.jointRotation[9 * k], R);
                for (int a = 0; a < 3; ++a) m.jointOrigin[3 * k + a] = m.jointOrigin[3 * j + a] + o[a];
                for (int a = 0; a < 9; ++a) m.jointRotation[9 * k + a] = R[a];
                m.parent[k] = P;
            }
        for (std::size_t f = 0; f < m.frameLink.size(); ++f)   // frames on c move to P
            if (m.frameLink[f] == c)
            {
                double p[3], R[9];
                rot(j, &m.framePose[12 * f], p);
                rotm(j, &m.framePose[12 * f + 3], R);
                for (int a = 0; a < 3; ++a) m.framePose[12 * f + a] = m.jointOrigin[3 * j + a] + p[a];
                for (int a = 0; a < 9; ++a) m.framePose[12 * f + 3 + a] = R[a];
                m.frameLink[f] = P;
            }
        // drop joint j and link c; links above c shift down by one
        m.parent.erase(m.parent.begin() + j);
        m.jointOrigin.erase(m.jointOrigin.begin() + 3 * j, m.jointOrigin.begin() + 3 * j + 3);
        m.jointRotation.erase(m.jointRotation.begin() + 9 * j, m.jointRotation.begin() + 9 * j + 9);
        m.jointAxis.erase(m.jointAxis.begin() + 3 * j, m.jointAxis.begin() + 3 * j + 3);
        if (m.jointType.size() == static_cast<std::size_t>(m.ndof)) m.jointType.erase(m.jointType.begin() + j);
        for (std::vector<double>* lim : {&m.jointLower, &m.jointUpper, &m.jointVelocityLimit})
            if (lim->size() == static_cast<std::size_t>(m.ndof)) lim->erase(lim->begin() + j);
        m.linkMass.erase(m.linkMass.begin() + c);
        m.linkCom.erase(m.linkCom.begin() + 3 * c, m.linkCom.begin() + 3 * c + 3);
        m.linkInertia.erase(m.linkInertia.begin() + 9 * c, m.linkInertia.begin() + 9 * c + 9);
        for (auto& p : m.parent)
            if (p > c) --p;
        for (auto& l : m.frameLink)
            if (l > c) --l;
        --m.ndof;
    }
    return m;
}

const char* describe(ModelDefect defect)
{
    switch (defect)
    {
    case ModelDefect::Corrupted: return "Corrupted robot model.";
    case ModelDefect::NotTopological: return "The joints must be in topological order (parent[j] <= j).";
    case ModelDefect::FrameOnUnknownLink: return "A frame is attached to a link the model does not have.";
    case ModelDefect::UnknownJointType: return "Unknown joint type";
    case ModelDefect::None: break;
    }
    return "";
}

std::string describe(ModelDefect defect, const RobotModel& reduced)
{
    std::string text = describe(defect);
    if (defect != ModelDefect::UnknownJointType) return text;
    for (const int32_t t : reduced.jointType)
        if (t != BLF_JOINT_REVOLUTE && t != BLF_JOINT_PRISMATIC)
            return text + " " + std::to_string(t) + " (revolute or prismatic; fixed joints go in fixedJoint).";
    return text + ".";
}

ModelDefect prepareRobotModel(const RobotModel& full, RobotModel& reduced)
{
    if (!full.fixedJoint.empty())
        if (const ModelDefect d = mergeDefect(full); d != ModelDefect::None) return d;
    reduced = full.fixedJoint.empty() ? full : reduceFixedJoints(full);
    if (reduced.ndof < 1 || reduced.ndof > BLF_FBD_MAX_DOFS) return ModelDefect::Corrupted;
    const std::size_t n = static_cast<std::size_t>(reduced.ndof);
    if (!sizesConsistent(reduced, n) || reduced.jointLower.size() != reduced.jointUpper.size()
        || !reduced.fixedJoint.empty())
        return ModelDefect::Corrupted;
    if (const ModelDefect d = orderAndFrames(reduced, n); d != ModelDefect::None) return d;
    for (const int32_t t : reduced.jointType)
        if (t != BLF_JOINT_REVOLUTE && t != BLF_JOINT_PRISMATIC) return ModelDefect::UnknownJointType;
    return ModelDefect::None;
}

bool DeviceRobotModel::set(const RobotModel& reduced)
{
    m_host = reduced;
    // an empty jointType frees its buffer, so the view's joint_type is null
    m_ok = m_d.parent.upload(reduced.parent) && m_d.origin.upload(reduced.jointOrigin)
           && m_d.rot.upload(reduced.jointRotation) && m_d.axis.upload(reduced.jointAxis)
           && m_d.mass.upload(reduced.linkMass) && m_d.com.upload(reduced.linkCom)
           && m_d.inertia.upload(reduced.linkInertia) && m_d.frameLink.upload(reduced.frameLink)
           && m_d.framePose.upload(reduced.framePose) && m_d.jointType.upload(reduced.jointType);
    return m_ok;
}

blf_fb_model DeviceRobotModel::view(const double gravity[3], double rho) const
{
    blf_fb_model d{};
    d.ndof = m_host.ndof;
    d.nframes = static_cast<int32_t>(m_host.frameLink.size());
    d.parent = m_d.parent.data();
    d.joint_origin = m_d.origin.data();
    d.joint_rot = m_d.rot.data();
    d.joint_axis = m_d.axis.data();
    d.link_mass = m_d.mass.data();
    d.link_com = m_d.com.data();
    d.link_inertia = m_d.inertia.data();
    d.frame_link = m_d.frameLink.data();
    d.frame_pose = m_d.framePose.data();
    std::copy(gravity, gravity + 3, d.gravity);
    d.rho = rho;
    d.joint_type = m_d.jointType.data();
    return d;
}

void fbStatePack(const Vector6& baseVel, const VectorXd& jointVel, const Vector3& basePos,
                 const Matrix3& baseRot, const VectorXd& jointPos, double* s)
{
    const std::size_t n = jointVel.size();
    const blf_fb_state at = fbStateAt(s, n);
    std::copy(baseVel.begin(), baseVel.end(), at.base_vel);
    std::copy(jointVel.data(), jointVel.data() + n, at.joint_vel);
    std::copy(basePos.begin(), basePos.end(), at.base_pos);
    std::copy(baseRot.begin(), baseRot.end(), at.base_rot);
    std::copy(jointPos.data(), jointPos.data() + n, at.joint_pos);
}

void fbStateUnpack(const double* s, std::size_t n, Vector6& baseVel, VectorXd& jointVel,
                   Vector3& basePos, Matrix3& baseRot, VectorXd& jointPos)
{
    const blf_fb_state at = fbStateAt(const_cast<double*>(s), n);   // read only
    std::copy(at.base_vel, at.base_vel + 6, baseVel.begin());
    jointVel.resize(n);
    std::copy(at.joint_vel, at.joint_vel + n, jointVel.data());
    std::copy(at.base_pos, at.base_pos + 3, basePos.begin());
    std::copy(at.base_rot, at.base_rot + 9, baseRot.begin());
    jointPos.resize(n);
    std::copy(at.joint_pos, at.joint_pos + n, jointPos.data());
}
} // namespace blf
