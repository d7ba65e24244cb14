// Stand-ins of the m-estimators of gtsam/linear/LossFunctions.h (GTSAM 4.2.0, as recalled) beside the Huber of mock_all.h: each has
// the constant behind modelParameter(), as the real classes do.  DCS is here as an m-estimator include/DynoGfxAdapter.hpp refuses.
// TEST INFRASTRUCTURE ONLY; no arithmetic.
#pragma once
#include <gtsam/mock_all.h>
namespace gtsam {
namespace noiseModel {
namespace mEstimator {
struct Fair : Base { double c = 0; double modelParameter() const { return c; } };
struct Cauchy : Base { double k = 0; double modelParameter() const { return k; } };
struct Tukey : Base { double c = 0; double modelParameter() const { return c; } };
struct Welsch : Base { double c = 0; double modelParameter() const { return c; } };
struct GemanMcClure : Base { double c = 0; double modelParameter() const { return c; } };
struct DCS : Base { double c = 0; double modelParameter() const { return c; } };
}  // namespace mEstimator
}  // namespace noiseModel
}  // namespace gtsam
