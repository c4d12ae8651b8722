/**
 * @file invdyn_tests.cpp
 * Tests of System::FloatingBaseDynamicalSystem::inverseDynamics, with ik_tests.cpp's conventions
 * ("name ... ok", "N checks, 0 failed"; modes cpu / gpu / all):
 *   cpu: without a robot model the call is refused with its line on std::cerr and leaves its outputs
 *        alone;
 *   gpu: on a 3-joint chain with a ContinuousContactModel foot, the torques of inverseDynamics set as the
 *        control input make dynamics() return the requested joint accelerations and the same base
 *        acceleration; without contacts, at rest and with zero accelerations they hold the joints
 *        against gravity while the base falls with g; a wrong size and a non-finite state are refused.
 */
#include <cmath>
#include <cstdio>
#include <functional>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include <BipedalLocomotion/ContactModels/ContinuousContactModel.h>
#include <BipedalLocomotion/ParametersHandler/IParametersHandler.h>
#include <BipedalLocomotion/System/FloatingBaseSystemDynamics.h>

#include "model_fixtures.h"
#include "test_harness.h"

using namespace BipedalLocomotion;
using namespace BipedalLocomotion::System;

static void testRefusedWithoutModel()
{
    FloatingBaseDynamicalSystem empty;
    blf::VectorXd acc(3, 0.0), tau(2, 7.0);
    blf::Vector6 base{};
    base[2] = 7.0;
    REQUIRE_FALSE(empty.inverseDynamics(acc, base, tau));
    REQUIRE(tau.size() == 2 && tau[0] == 7.0 && base[2] == 7.0);
}

static void testRoundTripOnDevice()
{
    auto system = std::make_shared<FloatingBaseDynamicalSystem>();
    auto handler = std::make_shared<ParametersHandler::StdImplementation>();
    handler->setParameter("rho", 0.01);
    REQUIRE(system->initalize(handler));
    REQUIRE(system->setRobotModel(chainModel()));
    const blf::Matrix3 R0 = blf::Transform::Identity().rotation;
    blf::VectorXd q(3, 0.0), qd(3, 0.0), zero3(3, 0.0);
    q[0] = 0.2; q[1] = -0.4; q[2] = 0.3;
    qd[0] = 0.5; qd[1] = -0.3; qd[2] = 0.8;
    blf::Vector6 nuB{};
    nuB[0] = 0.1; nuB[2] = -0.2; nuB[4] = 0.3;
    auto contact = std::make_shared<ContactModels::ContinuousContactModel>();
    auto cp = std::make_shared<ParametersHandler::StdImplementation>();
    cp->setParameter("length", 0.12);
    cp->setParameter("width", 0.09);
    cp->setParameter("spring_coeff", 3.0e4);
    cp->setParameter("damper_coeff", 300.0);
    REQUIRE(contact->initialize(cp));
    blf::Transform nullT;
    nullT.position = {{0.0, 0.0, 0.5}};
    contact->setNullForceTransform(nullT);
    REQUIRE(system->setState({nuB, qd, blf::Vector3{{0.0, 0.0, 1.0}}, R0, q}));
    REQUIRE(system->setControlInput({zero3, {ContactWrench(0, contact)}}));
    blf::VectorXd want(3, 0.0), tau;
    want[0] = 1.5; want[1] = -2.0; want[2] = 0.7;
    blf::Vector6 baseAcc{};
    REQUIRE(system->inverseDynamics(want, baseAcc, tau));
    REQUIRE(tau.size() == 3);
    REQUIRE(system->setControlInput({tau, {ContactWrench(0, contact)}}));
    FloatingBaseDynamicalSystem::StateDerivativeType dx;
    REQUIRE(system->dynamics(0.0, dx));
    for (int i = 0; i < 3; ++i) REQUIRE(std::abs(std::get<1>(dx)[i] - want[i]) < 1e-9);
    for (int i = 0; i < 6; ++i) REQUIRE(std::abs(std::get<0>(dx)[i] - baseAcc[i]) < 1e-9);
    // at rest, no contact, zero joint accelerations: the base falls with g and the torques hold the
    // joints still in the falling frame, i.e. they vanish
    REQUIRE(system->setState({blf::Vector6{}, zero3, blf::Vector3{{0.0, 0.0, 1.0}}, R0, q}));
    REQUIRE(system->setControlInput({zero3, {}}));
    REQUIRE(system->inverseDynamics(zero3, baseAcc, tau));
    REQUIRE(std::abs(baseAcc[2] + 9.81) < 1e-10);
    for (int i : {0, 1, 3, 4, 5}) REQUIRE(std::abs(baseAcc[i]) < 1e-10);
    for (int i = 0; i < 3; ++i) REQUIRE(std::abs(tau[i]) < 1e-10);
    // refusals: a wrong size, and a robot the device reports as failed
    REQUIRE_FALSE(system->inverseDynamics(blf::VectorXd(2, 0.0), baseAcc, tau));
    blf::VectorXd bad = q;
    bad[1] = std::numeric_limits<double>::quiet_NaN();
    REQUIRE(system->setState({blf::Vector6{}, zero3, blf::Vector3{{0.0, 0.0, 1.0}}, R0, bad}));
    tau[0] = 7.0;
    REQUIRE_FALSE(system->inverseDynamics(zero3, baseAcc, tau));
    REQUIRE(tau[0] == 7.0);
}

int main(int argc, char** argv)
{
    return runCases(argc, argv, {
        {"FloatingBaseDynamicalSystem inverseDynamics refusals", false, testRefusedWithoutModel},
        {"FloatingBaseDynamicalSystem inverseDynamics on the device", true, testRoundTripOnDevice},
    });
}
