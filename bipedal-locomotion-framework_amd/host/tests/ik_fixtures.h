/**
 * @file ik_fixtures.h
 * The 13-joint biped and the task makers that ik_hard_tests.cpp, ik_limits_tests.cpp and
 * ik_priority_tests.cpp share.  Each program's Biped / makeBiped (the task set it adds) stays with it;
 * ik_tests.cpp has a 7-joint model and parameterised makers of its own.
 */
#pragma once

#include <memory>
#include <vector>

#include <BipedalLocomotion/IK/QPInverseKinematics.h>
#include <BipedalLocomotion/ParametersHandler/IParametersHandler.h>

static constexpr int kJoints = 13;

inline std::shared_ptr<BipedalLocomotion::IK::SE3Task> se3Task(int frame)
{
    auto h = std::make_shared<BipedalLocomotion::ParametersHandler::StdImplementation>();
    h->setParameter("frame_index", frame);
    h->setParameter("kp_linear", 4.0);
    h->setParameter("kp_angular", 3.0);
    auto t = std::make_shared<BipedalLocomotion::IK::SE3Task>();
    t->initialize(h);
    return t;
}

inline std::shared_ptr<BipedalLocomotion::IK::CoMTask> comTask()
{
    auto h = std::make_shared<BipedalLocomotion::ParametersHandler::StdImplementation>();
    h->setParameter("kp_linear", 2.0);
    auto t = std::make_shared<BipedalLocomotion::IK::CoMTask>();
    t->initialize(h);
    return t;
}

inline std::shared_ptr<BipedalLocomotion::IK::JointTrackingTask> jointTask()
{
    auto h = std::make_shared<BipedalLocomotion::ParametersHandler::StdImplementation>();
    h->setParameter("kp", std::vector<double>(kJoints, 1.5));
    auto t = std::make_shared<BipedalLocomotion::IK::JointTrackingTask>();
    t->initialize(h);
    return t;
}

// pelvis, two legs of six joints (hip yaw / roll / pitch, knee, ankle pitch / roll), one torso joint;
// sole frames on the feet.  (ik_tests.cpp's biped has three joints per leg: with both soles planted it
// is a closed chain with a redundant constraint, so its twelve foot rows are dependent.)
inline blf::RobotModel bipedModel()
{
    blf::RobotModel m;
    m.ndof = kJoints;
    m.parent = {0, 1, 2, 3, 4, 5, 0, 7, 8, 9, 10, 11, 0};
    for (double side : {0.08, -0.08})
        m.jointOrigin.insert(m.jointOrigin.end(), {0.0, side, -0.05, 0.0, 0.0, -0.02, 0.0, 0.0, -0.02,
                                                   0.0, 0.0, -0.25, 0.0, 0.0, -0.25, 0.0, 0.0, -0.02});
    m.jointOrigin.insert(m.jointOrigin.end(), {0.0, 0.0, 0.1});
    for (int j = 0; j < kJoints; ++j) m.jointRotation.insert(m.jointRotation.end(), {1, 0, 0, 0, 1, 0, 0, 0, 1});
    for (int leg = 0; leg < 2; ++leg)
        m.jointAxis.insert(m.jointAxis.end(), {0, 0, 1, 1, 0, 0, 0, 1, 0, 0, 1, 0, 0, 1, 0, 1, 0, 0});
    m.jointAxis.insert(m.jointAxis.end(), {0, 0, 1});
    m.linkMass = {6.0, 1.0, 0.5, 2.0, 1.5, 0.3, 0.8, 1.0, 0.5, 2.0, 1.5, 0.3, 0.8, 5.0};
    m.linkCom = {0.0, 0.0, 0.02};
    for (int leg = 0; leg < 2; ++leg)
        m.linkCom.insert(m.linkCom.end(), {0.0, 0.0, -0.01, 0.0, 0.0, -0.01, 0.0, 0.0, -0.12,
                                           0.0, 0.0, -0.12, 0.0, 0.0, -0.01, 0.03, 0.0, -0.02});
    m.linkCom.insert(m.linkCom.end(), {0.0, 0.0, 0.15});
    for (double mass : m.linkMass)
        m.linkInertia.insert(m.linkInertia.end(), {0.01 * mass, 0, 0, 0, 0.012 * mass, 0, 0, 0, 0.008 * mass});
    m.frameLink = {6, 12};
    m.framePose = {0.02, 0.0, -0.04, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0.02, 0.0, -0.04, 1, 0, 0, 0, 1, 0, 0, 0, 1};
    return m;
}
