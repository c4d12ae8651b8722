/**
 * @file RecursiveLeastSquare.h
 * The recursive-least-squares filter of src/Estimators/include/BipedalLocomotion/Estimators/
 * RecursiveLeastSquare.h:28-111 (Ljung, System Identification, 11.2): the same public methods,
 * parameter keys and state machine; every advance() is one blf_rls_advance (include/blf/blf_c.h
 * section 10) with one filter and one step on the calling thread's library handle.
 *
 * Differences from the reference a user can notice: vectors are std::vector<double> and matrices
 * are row-major std::vector<double> (the regressor function returns its m x n matrix that way,
 * parametersCovarianceMatrix() is n x n); the gain is applied as m sequential scalar updates
 * instead of through an explicit m x m inverse (the same estimate up to rounding);
 * the state and the measurements hold at most 8 elements each; a regressor of the wrong size makes
 * advance() return false (the reference asserts inside Eigen).
 */
#ifndef BLF_BIPEDAL_LOCOMOTION_ESTIMATORS_RLS_H
#define BLF_BIPEDAL_LOCOMOTION_ESTIMATORS_RLS_H

#include <functional>
#include <memory>
#include <vector>

#include <BipedalLocomotion/ParametersHandler/IParametersHandler.h>
#include <blf/device.h>

namespace BipedalLocomotion
{
namespace Estimators
{

class RecursiveLeastSquare
{
public:
    /**
     * Read the filter's settings: "measurement_covariance" (the diagonal of the measurements'
     * covariance, m values), "lambda" (the forgetting factor; 1 makes the filter a Kalman filter),
     * "state" (the initial estimate, n values) and "state_covariance" (the diagonal of its
     * covariance).  False if the filter was initialised before, the handler is expired or a key is
     * missing.
     */
    bool initialize(std::weak_ptr<ParametersHandler::IParametersHandler> handlerWeak);

    /** The function returning the m x n regressor (row-major) of the current sample. */
    void setRegressorFunction(std::function<std::vector<double>(void)> regressor);

    /** The m measurements of the current sample. */
    void setMeasurements(const std::vector<double>& measurements);

    /** One step of the filter; false before initialize() or setRegressorFunction(). */
    bool advance();

    const std::vector<double>& parametersExpectedValue() const;

    /** n x n, row-major. */
    const std::vector<double>& parametersCovarianceMatrix() const;

private:
    enum class State
    {
        NotInitialized,
        Initialized,
        Running
    };

    std::vector<double> m_state;
    std::vector<double> m_measurements;
    std::vector<double> m_stateCovarianceMatrix;       // n x n row-major
    std::vector<double> m_measurementCovariance;       // the diagonal
    double m_lambda{1.0};
    std::function<std::vector<double>(void)> m_regressor;
    State m_estimatorState{State::NotInitialized};

    std::vector<double> m_staging;                     // host image of m_device
    blf::DeviceBuffer<double> m_device;                // r m | H m n | y m | x n | P n n
};

} // namespace Estimators
} // namespace BipedalLocomotion

#endif // BLF_BIPEDAL_LOCOMOTION_ESTIMATORS_RLS_H
