/**
 * @file rls_tests.cpp
 * Tests of the Estimators::RecursiveLeastSquare adapter, with host_tests.cpp's conventions
 * ("name ... ok", "N checks, 0 failed"; modes cpu / gpu / all):
 *   cpu: every path on which the adapter returns false without touching a device, and the
 *        ingestion of the reference's Estimators test configuration (tests/golden/
 *        estimators_config.ini) through StdImplementation::setFromFile;
 *   gpu: src/Estimators/tests/RecursiveLeastSquareTest.cpp:36-142 restated: the two-parameter
 *        model with std::mt19937{42} noise, 10 000 advance() calls, 0.1 % on both parameters.
 */
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include <BipedalLocomotion/Estimators/RecursiveLeastSquare.h>
#include <BipedalLocomotion/ParametersHandler/IParametersHandler.h>

#include "test_harness.h"

using namespace BipedalLocomotion::Estimators;
using namespace BipedalLocomotion::ParametersHandler;

static std::string g_golden = "tests/golden";

static std::shared_ptr<StdImplementation> fullHandler()
{
    auto h = std::make_shared<StdImplementation>();
    h->setParameter("lambda", 1.0);
    h->setParameter("measurement_covariance", std::vector<double>{0.5, 0.5});
    h->setParameter("state", std::vector<double>{0.0, 0.0});
    h->setParameter("state_covariance", std::vector<double>{10.0, 10.0});
    return h;
}

static std::shared_ptr<StdImplementation> handlerWithout(const std::string& key)
{
    auto h = std::make_shared<StdImplementation>();
    if (key != "lambda") h->setParameter("lambda", 1.0);
    if (key != "measurement_covariance")
        h->setParameter("measurement_covariance", std::vector<double>{0.5, 0.5});
    if (key != "state") h->setParameter("state", std::vector<double>{0.0, 0.0});
    if (key != "state_covariance") h->setParameter("state_covariance", std::vector<double>{10.0, 10.0});
    return h;
}

static void testStateMachine()
{
    // advance before setRegressorFunction, initialised or not
    {
        RecursiveLeastSquare rls;
        REQUIRE_FALSE(rls.advance());
        REQUIRE(rls.initialize(fullHandler()));
        REQUIRE_FALSE(rls.advance());
    }
    // advance before initialize
    {
        RecursiveLeastSquare rls;
        rls.setRegressorFunction([] { return std::vector<double>(4, 1.0); });
        REQUIRE_FALSE(rls.advance());
    }
    // a second initialize
    {
        RecursiveLeastSquare rls;
        REQUIRE(rls.initialize(fullHandler()));
        REQUIRE_FALSE(rls.initialize(fullHandler()));
        REQUIRE(rls.parametersExpectedValue() == (std::vector<double>{0.0, 0.0}));
        REQUIRE(rls.parametersCovarianceMatrix() == (std::vector<double>{10.0, 0.0, 0.0, 10.0}));
    }
    // an expired handler; the filter stays uninitialised and can be initialised afterwards
    {
        RecursiveLeastSquare rls;
        std::weak_ptr<IParametersHandler> expired;
        {
            auto temporary = fullHandler();
            expired = temporary;
        }
        REQUIRE_FALSE(rls.initialize(expired));
        REQUIRE(rls.initialize(fullHandler()));
    }
    // each missing key
    for (const char* key : {"measurement_covariance", "lambda", "state", "state_covariance"})
    {
        RecursiveLeastSquare rls;
        REQUIRE_FALSE(rls.initialize(handlerWithout(key)));
    }
    // sizes outside what the device filter is built for
    {
        auto h = fullHandler();
        h->setParameter("state", std::vector<double>(9, 0.0));
        h->setParameter("state_covariance", std::vector<double>(9, 1.0));
        RecursiveLeastSquare rls;
        REQUIRE_FALSE(rls.initialize(h));
        auto g = fullHandler();
        g->setParameter("measurement_covariance", std::vector<double>(9, 1.0));
        REQUIRE_FALSE(rls.initialize(g));
    }
    // a regressor of the wrong size is refused before any device work
    {
        RecursiveLeastSquare rls;
        REQUIRE(rls.initialize(fullHandler()));
        rls.setRegressorFunction([] { return std::vector<double>(3, 1.0); });
        REQUIRE_FALSE(rls.advance());
    }
}

static void testConfigFile()
{
    auto handler = std::make_shared<StdImplementation>();
    REQUIRE(handler->setFromFile(g_golden + "/estimators_config.ini"));
    double lambda = 0.0;
    std::vector<double> v;
    REQUIRE(handler->getParameter("lambda", lambda));
    REQUIRE(lambda == 1.0);
    REQUIRE(handler->getParameter("measurement_covariance", v));
    REQUIRE(v == (std::vector<double>{0.5, 0.5}));
    RecursiveLeastSquare rls;
    REQUIRE(rls.initialize(handler));
    REQUIRE(rls.parametersExpectedValue() == (std::vector<double>{0.0, 0.0}));
    REQUIRE(rls.parametersCovarianceMatrix() == (std::vector<double>{10.0, 0.0, 0.0, 10.0}));
}

// |y1|   |x      x * x |   |p1|   |noise_1|
// |y2| = |sin(x) cos(x)| * |p2| + |noise_2|
struct Model
{
    double p[2];
    double x{0.0};
    std::mt19937 gen{42};
    std::normal_distribution<> noise1{0, 0.5};
    std::normal_distribution<> noise2{0, 0.5};

    std::vector<double> regressor() const { return {x, x * x, std::sin(x), std::cos(x)}; }
    std::vector<double> output()
    {
        const std::vector<double> H = regressor();
        std::vector<double> y = {H[0] * p[0] + H[1] * p[1], H[2] * p[0] + H[3] * p[1]};
        y[0] += noise1(gen);
        y[1] += noise2(gen);
        return y;
    }
};

static void testRecursiveLeastSquare()
{
    Model model{{43.2, 12.2}};
    auto handler = std::make_shared<StdImplementation>();
    REQUIRE(handler->setFromFile(g_golden + "/estimators_config.ini"));
    RecursiveLeastSquare estimator;
    REQUIRE(estimator.initialize(handler));
    estimator.setRegressorFunction(std::bind(&Model::regressor, &model));
    bool advanced = true;
    for (int i = 0; i < 10000 && advanced; i++)
    {
        model.x = std::cos(i / 10.0);
        estimator.setMeasurements(model.output());
        advanced = estimator.advance();
    }
    REQUIRE(advanced);
    const double admissibleError = 0.1 / 100.0;
    const std::vector<double>& est = estimator.parametersExpectedValue();
    REQUIRE(std::abs((est[0] - model.p[0]) / model.p[0]) < admissibleError);
    REQUIRE(std::abs((est[1] - model.p[1]) / model.p[1]) < admissibleError);
    const std::vector<double>& P = estimator.parametersCovarianceMatrix();
    REQUIRE(P.size() == 4);
    REQUIRE(P[1] == P[2]);                                          // symmetric, exactly
    REQUIRE(P[0] > 0.0 && P[3] > 0.0 && P[0] * P[3] - P[1] * P[2] > 0.0);   // positive definite
}

int main(int argc, char** argv)
{
    if (const char* g = std::getenv("BLF_GOLDEN_DIR")) g_golden = g;
    return runCases(argc, argv, {
        {"RecursiveLeastSquare state machine", false, testStateMachine},
        {"RecursiveLeastSquare config.ini", false, testConfigFile},
        {"Recursive Least Square", true, testRecursiveLeastSquare},
    });
}
