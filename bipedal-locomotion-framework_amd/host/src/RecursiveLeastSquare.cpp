/**
 * @file RecursiveLeastSquare.cpp
 * Parameter handling, state machine and return values follow src/Estimators/src/
 * RecursiveLeastSquare.cpp:17-149; the update of :119-130 runs on the device through
 * blf_rls_advance (one filter, one step per advance()).
 */
#include <algorithm>
#include <iostream>

#include <BipedalLocomotion/Estimators/RecursiveLeastSquare.h>

using namespace BipedalLocomotion::Estimators;
using namespace BipedalLocomotion::ParametersHandler;

bool RecursiveLeastSquare::initialize(std::weak_ptr<IParametersHandler> handlerWeak)
{
    if (m_estimatorState != State::NotInitialized)
    {
        std::cerr << "[RecursiveLeastSquare::initialize] This filter is initialized already."
                  << std::endl;
        return false;
    }

    auto handler = handlerWeak.lock();
    if (handler == nullptr)
    {
        std::cerr << "[RecursiveLeastSquare::initialize] The parameters handler no longer exists."
                  << std::endl;
        return false;
    }

    // uncorrelated measurements: only the diagonal of their covariance is a parameter
    std::vector<double> measurementCovariance;
    if (!handler->getParameter("measurement_covariance", measurementCovariance))
    {
        std::cerr << "[RecursiveLeastSquare::initialize] The parameter measurement_covariance is "
                     "missing."
                  << std::endl;
        return false;
    }

    double lambda = 1.0;
    if (!handler->getParameter("lambda", lambda))
    {
        std::cerr << "[RecursiveLeastSquare::initialize] The parameter lambda is missing."
                  << std::endl;
        return false;
    }

    std::vector<double> state;
    if (!handler->getParameter("state", state))
    {
        std::cerr << "[RecursiveLeastSquare::initialize] The parameter state (the initial "
                     "estimate) is missing."
                  << std::endl;
        return false;
    }

    std::vector<double> stateCovariance;
    if (!handler->getParameter("state_covariance", stateCovariance))
    {
        std::cerr << "[RecursiveLeastSquare::initialize] The parameter state_covariance is missing."
                  << std::endl;
        return false;
    }

    const std::size_t n = state.size(), m = measurementCovariance.size();
    if (stateCovariance.size() != n)
    {
        std::cerr << "[RecursiveLeastSquare::initialize] state_covariance has "
                  << stateCovariance.size() << " elements, state has " << n << "." << std::endl;
        return false;
    }
    if (n < 1 || n > BLF_RLS_MAX_STATE || m < 1 || m > BLF_RLS_MAX_MEAS)
    {
        std::cerr << "[RecursiveLeastSquare::initialize] " << n << " parameters and " << m
                  << " measurements: the filter supports 1 to " << BLF_RLS_MAX_STATE << " and 1 to "
                  << BLF_RLS_MAX_MEAS << "." << std::endl;
        return false;
    }

    m_measurementCovariance = measurementCovariance;
    m_lambda = lambda;
    m_state = state;
    m_stateCovarianceMatrix.assign(n * n, 0.0);
    for (std::size_t i = 0; i < n; ++i) m_stateCovarianceMatrix[i * n + i] = stateCovariance[i];
    m_measurements.assign(m, 0.0);

    m_estimatorState = State::Initialized;
    return true;
}

void RecursiveLeastSquare::setRegressorFunction(std::function<std::vector<double>(void)> regressor)
{
    m_regressor = regressor;
}

void RecursiveLeastSquare::setMeasurements(const std::vector<double>& measurements)
{
    if (measurements.size() != m_measurements.size())
    {
        std::cerr << "[RecursiveLeastSquare::setMeasurements] " << measurements.size()
                  << " measurements given, " << m_measurements.size() << " expected; ignored."
                  << std::endl;
        return;
    }
    m_measurements = measurements;
}

bool RecursiveLeastSquare::advance()
{
    if (m_regressor == nullptr)
    {
        std::cerr << "[RecursiveLeastSquare::advance] No regressor function: call "
                     "setRegressorFunction() first."
                  << std::endl;
        return false;
    }
    if (m_estimatorState != State::Initialized && m_estimatorState != State::Running)
    {
        std::cerr << "[RecursiveLeastSquare::advance] The filter is not initialized: call "
                     "initialize() first."
                  << std::endl;
        return false;
    }

    const std::size_t n = m_state.size(), m = m_measurements.size();
    const std::vector<double> regressor = m_regressor();
    if (regressor.size() != m * n)
    {
        std::cerr << "[RecursiveLeastSquare::advance] The regressor has " << regressor.size()
                  << " elements, " << m << " x " << n << " expected." << std::endl;
        return false;
    }

    blf_handle* h = blf::threadHandle();
    if (h == nullptr)
    {
        std::cerr << "[RecursiveLeastSquare::advance] No device." << std::endl;
        return false;
    }

    if (m_estimatorState == State::Initialized) m_estimatorState = State::Running;

    // one upload (r | H | y | x | P), one launch, one download (x | P)
    const std::size_t oH = m, oY = oH + m * n, oX = oY + m, oP = oX + n, total = oP + n * n;
    m_staging.resize(total);
    std::copy(m_measurementCovariance.begin(), m_measurementCovariance.end(), m_staging.begin());
    std::copy(regressor.begin(), regressor.end(), m_staging.begin() + oH);
    std::copy(m_measurements.begin(), m_measurements.end(), m_staging.begin() + oY);
    std::copy(m_state.begin(), m_state.end(), m_staging.begin() + oX);
    std::copy(m_stateCovarianceMatrix.begin(), m_stateCovarianceMatrix.end(),
              m_staging.begin() + oP);
    if (!m_device.upload(m_staging)) return false;
    double* d = m_device.data();
    if (!blf::report(blf_rls_advance(h, static_cast<int32_t>(n), static_cast<int32_t>(m), m_lambda,
                                     d, 1, d + oH, d + oY, 1, d + oX, d + oP, 1, nullptr),
                     "RecursiveLeastSquare::advance"))
        return false;
    if (!m_device.download(m_staging.data(), total)) return false;
    std::copy(m_staging.begin() + oX, m_staging.begin() + oP, m_state.begin());
    std::copy(m_staging.begin() + oP, m_staging.end(), m_stateCovarianceMatrix.begin());
    return true;
}

const std::vector<double>& RecursiveLeastSquare::parametersExpectedValue() const
{
    return m_state;
}

const std::vector<double>& RecursiveLeastSquare::parametersCovarianceMatrix() const
{
    return m_stateCovarianceMatrix;
}
