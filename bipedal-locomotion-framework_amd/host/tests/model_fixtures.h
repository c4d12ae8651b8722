/**
 * @file model_fixtures.h
 * The 3-joint chain that host_tests.cpp, invdyn_tests.cpp and model_tests.cpp share (the 13-joint
 * biped is ik_fixtures.h's).
 */
#pragma once

#include <blf/robot_model.h>

// base, three links hanging below one another (joint axes x, y, y), a sole frame on the last link
inline blf::RobotModel chainModel()
{
    blf::RobotModel m;
    m.ndof = 3;
    m.parent = {0, 1, 2};
    m.jointOrigin = {0.0, 0.0, -0.1, 0.0, 0.0, -0.3, 0.0, 0.0, -0.3};
    for (int j = 0; j < 3; ++j) m.jointRotation.insert(m.jointRotation.end(), {1, 0, 0, 0, 1, 0, 0, 0, 1});
    m.jointAxis = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 1.0, 0.0};
    m.linkMass = {5.0, 2.0, 1.5, 1.0};
    m.linkCom = {0.0, 0.0, 0.0, 0.0, 0.0, -0.15, 0.0, 0.0, -0.15, 0.05, 0.0, -0.02};
    for (double mass : m.linkMass)
        m.linkInertia.insert(m.linkInertia.end(), {0.01 * mass, 0, 0, 0, 0.012 * mass, 0, 0, 0, 0.008 * mass});
    m.frameLink = {3};
    m.framePose = {0.02, 0.0, -0.05, 1, 0, 0, 0, 1, 0, 0, 0, 1};
    return m;
}
