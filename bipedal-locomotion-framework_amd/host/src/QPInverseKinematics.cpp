/**
 * @file QPInverseKinematics.cpp
 * The task bookkeeping of IK::QPInverseKinematics on the host; every advance() is one
 * blf_fb_ik_solve, with hard tasks blf_fb_ik_solve_hard, with a JointLimitsTask
 * blf_fb_ik_solve_limits, for one robot (include/blf/blf_c.h sections 12, 12b and 12c).
 */
#include <algorithm>
#include <cmath>
#include <iostream>

#include <BipedalLocomotion/IK/QPInverseKinematics.h>

using namespace BipedalLocomotion::IK;
using namespace BipedalLocomotion::ParametersHandler;

bool QPInverseKinematics::initialize(std::weak_ptr<IParametersHandler> handlerWeak)
{
    auto handler = handlerWeak.lock();
    if (handler == nullptr)
    {
        std::cerr << "[QPInverseKinematics::initialize] The parameters handler no longer exists."
                  << std::endl;
        return false;
    }
    double damping = 0.0;
    if (handler->getParameter("base_damping", damping) && (!std::isfinite(damping) || damping < 0.0))
    {
        std::cerr << "[QPInverseKinematics::initialize] The base_damping must be a non-negative number."
                  << std::endl;
        return false;
    }
    double hardWeight = 1.0;
    if (handler->getParameter("hard_task_weight", hardWeight) && (!std::isfinite(hardWeight) || hardWeight <= 0.0))
    {
        std::cerr << "[QPInverseKinematics::initialize] The hard_task_weight must be a positive number."
                  << std::endl;
        return false;
    }
    m_baseDamping = damping;
    m_hardWeight = hardWeight;
    return true;
}

bool QPInverseKinematics::setRobotModel(const blf::RobotModel& fullModel,
                                        const std::vector<std::string>& frameNames)
{
    constexpr const char* where = "[QPInverseKinematics::setRobotModel] ";
    m_hasModel = false;
    m_isValid = false;
    if (m_isFinalized)
    {
        std::cerr << where << "The problem is already finalized." << std::endl;
        return false;
    }
    blf::RobotModel model;
    const blf::ModelDefect defect = blf::prepareRobotModel(fullModel, model);
    if (defect != blf::ModelDefect::None)
    {
        std::cerr << where << blf::describe(defect, model) << std::endl;
        return false;
    }
    if (!frameNames.empty() && frameNames.size() != model.frameLink.size())
    {
        std::cerr << where << frameNames.size() << " frame names for " << model.frameLink.size() << " frames."
                  << std::endl;
        return false;
    }
    if (blf::threadHandle() == nullptr)
    {
        std::cerr << where << "No device." << std::endl;
        return false;
    }
    m_frameNames = frameNames;
    m_hasModel = m_model.set(model);
    return m_hasModel;
}

bool QPInverseKinematics::setRobotState(const blf::Vector3& basePosition, const blf::Matrix3& baseRotation,
                                        const blf::VectorXd& jointPositions)
{
    if (!m_hasModel)
    {
        std::cerr << "[QPInverseKinematics::setRobotState] Please call 'setRobotModel()' before."
                  << std::endl;
        return false;
    }
    if (jointPositions.size() != static_cast<std::size_t>(m_model.host().ndof))
    {
        std::cerr << "[QPInverseKinematics::setRobotState] Wrong size of the vectors." << std::endl;
        return false;
    }
    m_basePosition = basePosition;
    m_baseRotation = baseRotation;
    m_jointPositions = jointPositions;
    m_hasState = true;
    return true;
}

bool QPInverseKinematics::addTask(std::shared_ptr<IKLinearTask> task, const std::string& taskName,
                                  unsigned int priority, const blf::VectorXd& weight)
{
    constexpr const char* where = "[QPInverseKinematics::addTask] ";
    if (m_isFinalized)
    {
        std::cerr << where << "The problem is already finalized: no task can be added." << std::endl;
        return false;
    }
    if (task == nullptr)
    {
        std::cerr << where << "The task " << taskName << " is not valid (null pointer)." << std::endl;
        return false;
    }
    if (priority > 1)
    {
        std::cerr << where << "The task " << taskName << " has priority " << priority
                  << ": only hard (priority 0) and weighted (priority 1) tasks are supported." << std::endl;
        return false;
    }
    const bool hard = priority == 0;
    if (task->kind() == IKLinearTask::Kind::JointLimits && (!hard || m_limitsTask >= 0))
    {
        std::cerr << where << "The task " << taskName << " is a joint limits task: it is accepted at priority 0 "
                     "only, and once."
                  << std::endl;
        return false;
    }
    if (hard && weight.size() != 0)
    {
        std::cerr << where << "The task " << taskName << " has priority 0: a hard task takes no weight."
                  << std::endl;
        return false;
    }
    if (hard && task->kind() == IKLinearTask::Kind::JointTracking)
    {
        std::cerr << where << "The task " << taskName << " is the joint tracking task, the regulariser: it "
                     "cannot be hard (priority 0)."
                  << std::endl;
        return false;
    }
    for (const Entry& e : m_tasks)
        if (e.name == taskName)
        {
            std::cerr << where << "The task named " << taskName << " already exists." << std::endl;
            return false;
        }
    const IKLinearTask::Kind kind = task->kind();
    if (kind == IKLinearTask::Kind::JointLimits)
    {
        m_limitsTask = static_cast<int>(m_tasks.size());
        m_tasks.push_back(Entry{taskName, std::move(task), {}, true});
        return true;
    }
    std::size_t se3 = 0;
    for (const Entry& e : m_tasks) se3 += e.task->kind() == IKLinearTask::Kind::SE3;
    if (kind == IKLinearTask::Kind::SE3 && se3 >= BLF_IK_MAX_SE3_TASKS)
    {
        std::cerr << where << "At most " << BLF_IK_MAX_SE3_TASKS << " SE3 tasks are supported." << std::endl;
        return false;
    }
    if (kind == IKLinearTask::Kind::CoM && m_comTask >= 0)
    {
        std::cerr << where << "A CoM task already exists." << std::endl;
        return false;
    }
    if (kind == IKLinearTask::Kind::JointTracking && m_jointTask >= 0)
    {
        std::cerr << where << "A joint tracking task already exists." << std::endl;
        return false;
    }
    const bool joint = kind == IKLinearTask::Kind::JointTracking;
    const std::size_t rows = kind == IKLinearTask::Kind::SE3 ? 6 : kind == IKLinearTask::Kind::CoM ? 3 : weight.size();
    if (hard)
    {
        if (kind == IKLinearTask::Kind::CoM) m_comTask = static_cast<int>(m_tasks.size());
        m_tasks.push_back(Entry{taskName, std::move(task), std::vector<double>(rows, m_hardWeight), true});
        return true;
    }
    if (weight.size() != rows || rows == 0)
    {
        std::cerr << where << "The weight of the task " << taskName << " has " << weight.size()
                  << " entries; one per task row is required." << std::endl;
        return false;
    }
    for (std::size_t i = 0; i < rows; ++i)
        if (!std::isfinite(weight[i]) || weight[i] < 0.0 || (joint && weight[i] == 0.0))
        {
            std::cerr << where << "The weight of the task " << taskName << " must be finite and "
                      << (joint ? "positive." : "non-negative.") << std::endl;
            return false;
        }
    if (kind == IKLinearTask::Kind::CoM) m_comTask = static_cast<int>(m_tasks.size());
    if (joint) m_jointTask = static_cast<int>(m_tasks.size());
    m_tasks.push_back(Entry{taskName, std::move(task), std::vector<double>(weight.data(), weight.data() + rows),
                            false, true});
    return true;
}

bool QPInverseKinematics::setTaskPriority(const std::string& taskName, unsigned int priority)
{
    constexpr const char* where = "[QPInverseKinematics::setTaskPriority] ";
    if (priority > 1)
    {
        std::cerr << where << "The task " << taskName << " cannot get priority " << priority
                  << ": only hard (priority 0) and weighted (priority 1) tasks are supported." << std::endl;
        return false;
    }
    const auto it = std::find_if(m_tasks.begin(), m_tasks.end(), [&](const Entry& e) { return e.name == taskName; });
    if (it == m_tasks.end())
    {
        std::cerr << where << "The task named " << taskName << " does not exist." << std::endl;
        return false;
    }
    const IKLinearTask::Kind kind = it->task->kind();
    if (kind != IKLinearTask::Kind::SE3 && kind != IKLinearTask::Kind::CoM)
    {
        std::cerr << where << "The task " << taskName << " is not an SE3 or a CoM task: its priority is fixed."
                  << std::endl;
        return false;
    }
    if (!it->weighted)
    {
        std::cerr << where << "The task " << taskName << " was added at priority 0: it has no weights of its own "
                     "to return to, so its priority is fixed."
                  << std::endl;
        return false;
    }
    if (std::any_of(it->weight.begin(), it->weight.end(), [](double w) { return !(w > 0.0); }))
    {
        std::cerr << where << "The task " << taskName << " has a zero weight: a hard row needs a positive one."
                  << std::endl;
        return false;
    }
    it->hard = priority == 0;
    return true;
}

uint32_t QPInverseKinematics::hardRows() const
{
    uint32_t rows = 0;
    int k = 0;
    for (const Entry& e : m_tasks)
    {
        if (e.task->kind() == IKLinearTask::Kind::SE3)
        {
            if (e.hard) rows |= 0x3fu << (6 * k);   // (the joint limits task has no rows)
            ++k;
        }
        else if (e.task->kind() == IKLinearTask::Kind::CoM && e.hard)
            rows |= 0x7u << 24;
    }
    return rows;
}

std::vector<std::string> QPInverseKinematics::getTaskNames() const
{
    std::vector<std::string> names;
    for (const Entry& e : m_tasks) names.push_back(e.name);
    return names;
}

bool QPInverseKinematics::finalize()
{
    constexpr const char* where = "[QPInverseKinematics::finalize] ";
    if (!m_hasModel)
    {
        std::cerr << where << "Please call 'setRobotModel()' before." << std::endl;
        return false;
    }
    std::vector<int32_t> frames;
    for (const Entry& e : m_tasks)
    {
        if (e.task->kind() != IKLinearTask::Kind::SE3) continue;
        const auto& se3 = static_cast<const SE3Task&>(*e.task);
        int index = se3.frameIndex();
        if (!se3.frameName().empty())
        {
            const auto it = std::find(m_frameNames.begin(), m_frameNames.end(), se3.frameName());
            index = it == m_frameNames.end() ? -1 : static_cast<int>(it - m_frameNames.begin());
        }
        if (index < 0 || index >= static_cast<int>(m_model.host().frameLink.size()))
        {
            std::cerr << where << "The frame of the task " << e.name << " does not exist in the model."
                      << std::endl;
            return false;
        }
        frames.push_back(index);
    }
    if (m_jointTask >= 0 && m_tasks[m_jointTask].weight.size() != static_cast<std::size_t>(m_model.host().ndof))
    {
        std::cerr << where << "The joint tracking task's weight must have one entry per joint." << std::endl;
        return false;
    }
    std::vector<double> limits;
    if (m_limitsTask >= 0)
    {
        const auto& lt = static_cast<const JointLimitsTask&>(*m_tasks[m_limitsTask].task);
        const std::size_t n = static_cast<std::size_t>(m_model.host().ndof);
        if (!lt.isValid() || lt.klim().size() != n)
        {
            std::cerr << where << "The joint limits task " << m_tasks[m_limitsTask].name << " is not initialized "
                      << "or has " << lt.klim().size() << " joints, the model " << n << "." << std::endl;
            return false;
        }
        if (lt.useModelLimits() && m_model.host().jointLower.size() != n)
        {
            std::cerr << where << "The joint limits task asks for the model's limits and the model has none."
                      << std::endl;
            return false;
        }
        const std::vector<double>& lo = lt.useModelLimits() ? m_model.host().jointLower : lt.lowerLimits();
        const std::vector<double>& up = lt.useModelLimits() ? m_model.host().jointUpper : lt.upperLimits();
        limits.insert(limits.end(), lo.begin(), lo.end());
        limits.insert(limits.end(), up.begin(), up.end());
        limits.insert(limits.end(), lt.klim().begin(), lt.klim().end());
        limits.insert(limits.end(), lt.velocityLimits().begin(), lt.velocityLimits().end());
    }
    m_limits = limits;
    m_frames = frames;
    m_isFinalized = true;
    return true;
}

// device data layout (doubles): nu NV | state (bv 6 | jv n | bp 3 | bR 9 | jp n) | se3_weight 6K |
// se3_kp 2K | se3_pose 12K | se3_twist 6K | com_weight 3 | com_pos 3 | com_vel 3 | joint_weight n |
// joint_kp n | joint_pos n | joint_vel n; ints: frame K | status 1
bool QPInverseKinematics::advance()
{
    constexpr const char* where = "[QPInverseKinematics::advance] ";
    m_isValid = false;
    if (m_jointTask < 0)
    {
        std::cerr << where << "A joint tracking task is required: without it the problem is not "
                              "positive definite."
                  << std::endl;
        return false;
    }
    if (!m_isFinalized)
    {
        std::cerr << where << "Please call 'finalize()' before." << std::endl;
        return false;
    }
    if (!m_hasState)
    {
        std::cerr << where << "Please call 'setRobotState()' before." << std::endl;
        return false;
    }
    for (const Entry& e : m_tasks)
        if (!e.task->isValid())
        {
            std::cerr << where << "The task " << e.name << " is not initialized or has no set point."
                      << std::endl;
            return false;
        }
    const std::size_t n = static_cast<std::size_t>(m_model.host().ndof), NV = n + 6, K = m_frames.size();
    const auto& jt = static_cast<const JointTrackingTask&>(*m_tasks[m_jointTask].task);
    if (jt.kp().size() != n || jt.position().size() != n)
    {
        std::cerr << where << "The joint tracking task has " << jt.kp().size() << " joints, the model " << n
                  << "." << std::endl;
        return false;
    }
    const std::size_t oState = NV, oW = oState + blf::fbStateSize(n), oKp = oW + 6 * K, oPose = oKp + 2 * K,
                      oTwist = oPose + 12 * K, oCw = oTwist + 6 * K, oCp = oCw + 3, oCv = oCp + 3,
                      oJw = oCv + 3, oJk = oJw + n, oJp = oJk + n, oJv = oJp + n, total = oJv + n;
    std::vector<double> host(total, 0.0);
    blf::fbStatePack(blf::Vector6{}, blf::VectorXd(n), m_basePosition, m_baseRotation, m_jointPositions,
                     host.data() + oState);   // the velocities are not read
    std::size_t k = 0;
    for (const Entry& e : m_tasks)
    {
        if (e.task->kind() != IKLinearTask::Kind::SE3) continue;
        const auto& se3 = static_cast<const SE3Task&>(*e.task);
        std::copy(e.weight.begin(), e.weight.end(), host.begin() + oW + 6 * k);
        host[oKp + 2 * k] = se3.kpLinear();
        host[oKp + 2 * k + 1] = se3.kpAngular();
        const auto packed = se3.pose().packed();
        std::copy(packed.begin(), packed.end(), host.begin() + oPose + 12 * k);
        std::copy(se3.mixedVelocity().begin(), se3.mixedVelocity().end(), host.begin() + oTwist + 6 * k);
        ++k;
    }
    double comKp = 0.0;
    if (m_comTask >= 0)
    {
        const auto& com = static_cast<const CoMTask&>(*m_tasks[m_comTask].task);
        std::copy(m_tasks[m_comTask].weight.begin(), m_tasks[m_comTask].weight.end(), host.begin() + oCw);
        std::copy(com.position().begin(), com.position().end(), host.begin() + oCp);
        std::copy(com.velocity().begin(), com.velocity().end(), host.begin() + oCv);
        comKp = com.kpLinear();
    }
    std::copy(m_tasks[m_jointTask].weight.begin(), m_tasks[m_jointTask].weight.end(), host.begin() + oJw);
    std::copy(jt.kp().begin(), jt.kp().end(), host.begin() + oJk);
    for (std::size_t i = 0; i < n; ++i)
    {
        host[oJp + i] = jt.position()[i];
        host[oJv + i] = jt.velocity()[i];
    }
    std::vector<int32_t> ints(m_frames);
    ints.push_back(0);
    blf_handle* h = blf::threadHandle();
    if (h == nullptr)
    {
        std::cerr << where << "No device." << std::endl;
        return false;
    }
    if (!m_dData.upload(host) || !m_dInt.upload(ints)) return false;

    double* d = m_dData.data();
    const double gravity[3] = {0.0, 0.0, -9.81};
    m_cModel = m_model.view(gravity, 0.01);
    m_cState = blf::fbStateAt(d + oState, n);
    m_cTasks = blf_ik_tasks{};
    m_cTasks.nse3 = static_cast<int32_t>(K);
    m_cTasks.frame = m_dInt.data();
    m_cTasks.se3_weight = d + oW;
    m_cTasks.se3_kp = d + oKp;
    m_cTasks.se3_pose = d + oPose;
    m_cTasks.se3_twist = d + oTwist;
    m_cTasks.com_weight = m_comTask >= 0 ? d + oCw : nullptr;
    m_cTasks.com_kp = comKp;
    m_cTasks.com_pos = d + oCp;
    m_cTasks.com_vel = d + oCv;
    m_cTasks.joint_weight = d + oJw;
    m_cTasks.joint_kp = d + oJk;
    m_cTasks.joint_pos = d + oJp;
    m_cTasks.joint_vel = d + oJv;
    m_cTasks.base_damping = m_baseDamping;
    int32_t* status = m_dInt.data() + K;
    m_cHard = blf_ik_hard{};
    m_cHard.rows = hardRows();
    m_cLimits = blf_ik_limits{};
    if (m_limitsTask >= 0)
    {
        if (!m_dLimits.upload(m_limits)) return false;
        const auto& lt = static_cast<const JointLimitsTask&>(*m_tasks[m_limitsTask].task);
        m_cLimits.pos_lower = m_dLimits.data();
        m_cLimits.pos_upper = m_dLimits.data() + n;
        m_cLimits.klim = m_dLimits.data() + 2 * n;
        m_cLimits.vel_max = m_limits.size() == 4 * n ? m_dLimits.data() + 3 * n : nullptr;
        m_cLimits.sampling_time = lt.samplingTime();
    }
    const blf_status called =
        m_limitsTask >= 0 ? blf_fb_ik_solve_limits(h, &m_cModel, &m_cState, &m_cTasks,
                                                   m_cHard.rows != 0 ? &m_cHard : nullptr, &m_cLimits, 1, d, status,
                                                   nullptr, nullptr, nullptr)
        : m_cHard.rows != 0
            ? blf_fb_ik_solve_hard(h, &m_cModel, &m_cState, &m_cTasks, &m_cHard, 1, d, status, nullptr)
            : blf_fb_ik_solve(h, &m_cModel, &m_cState, &m_cTasks, 1, d, status, nullptr);
    if (!blf::report(called, "QPInverseKinematics::advance")) return false;
    std::vector<double> nu(NV);
    if (!m_dData.download(nu.data(), NV) || !m_dInt.download(ints.data(), K + 1)) return false;
    if (ints[K] != BLF_IK_OK)
    {
        std::cerr << where
                  << (ints[K] == BLF_IK_BAD_INPUT ? "The robot state or a set point is not finite."
                      : ints[K] == BLF_IK_HARD_DEPENDENT
                          ? "The hard tasks are linearly dependent, conflicting or more than the unknowns."
                      : ints[K] == BLF_IK_LIMITS_UNRESOLVED
                          ? "The joint limits conflict with the hard tasks, or the active-set iteration did not "
                            "resolve them."
                          : "The problem is not positive definite.")
                  << std::endl;
        return false;
    }
    for (int i = 0; i < 6; ++i) m_state.baseVelocity[i] = nu[i];
    m_state.jointVelocity.resize(n);
    for (std::size_t i = 0; i < n; ++i) m_state.jointVelocity[i] = nu[6 + i];
    m_isValid = true;
    return true;
}
