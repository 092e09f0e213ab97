"""dhcos -- MI355X-native Double-Heston + Merton-jump COS pricing and calibration.

Drop-in host API for the hot path of zenthepen/Option-Pricing-FFN-LBFGS:

    DoubleHeston                      src/models/double_heston.py
    DoubleHestonJumpCalibrator,       src/calibration/lbfgs_calibrator.py
    CalibrationResult
    generate_synthetic_calibrations   src/data/synthetic_generator.py
    implied_vol                       (new: Black-Scholes implied volatility of prices)
    calibrate_batch                   (new: many markets on one option grid, calibrated together;
                                       gradient="analytic" runs them on the exact loss gradient,
                                       method="lm" by Levenberg-Marquardt on the Gauss-Newton
                                       Hessian; result.uncertainty() gives the parameters'
                                       covariance, standard errors and conditioning)
    monte_carlo                       (new: path pricing of European, Asian and barrier options,
                                       with antithetic pairs and COS-priced control variates)
    monte_carlo_greeks                (new: their delta, gamma and v0 vegas with standard errors,
                                       from coupled paths in one walk)
    american_monte_carlo              (new: American and Bermudan options by least-squares Monte Carlo)
    FFNModel, train_ffn,              (new: the warm-start network of the reference's documents --
    train_ffn_on_generator,            trained in PyTorch on the generator's output, evaluated by
    fine_tune_ffn, price_features      one fused gfx950 launch; calibrate_batch(x0s=model) starts
                                       every market from its prediction)
    greeks                            (new: analytic delta, gamma, dual delta and v0 vegas of the
                                       COS price, one pass; the module itself is dhcos/greeks.py)
    greeks_full, local_vol            (new: greeks' planes and, from the same pass, the maturity,
                                       rate and dividend sensitivities, the dual gamma / density
                                       and Dupire's local volatility, on a (K, T) grid in one
                                       launch; dhcos/greeks_full.py)
    parameter_sensitivities           (new: the price's analytic sensitivity to each of the 13 model
                                       parameters, one pass; DoubleHestonJumpCalibrator(...,
                                       gradient="analytic") fits with the exact loss gradient)

All pricing arithmetic runs in libdhcos.so (hand-written gfx950 HIP kernels, C-ABI in
include/dhcos.h); the native library is loaded on first use and there is no CPU fallback.
The reference's module names (double_heston, lbfgs_calibrator, synthetic_generator) sit next to
this package as one-line re-exports, and ``dhcos.distributed`` (import it explicitly; it needs
torch) shards starts / samples over ``torch.distributed`` ranks (one process per GPU).
"""
from .pricer import DoubleHeston, implied_vol
from .calibrator import CalibrationResult, DoubleHestonJumpCalibrator
from .generator import generate_synthetic_calibrations
from .batch import BatchCalibrationResult, ParameterUncertainty, calibrate_batch
from .montecarlo import (MonteCarloGreeks, MonteCarloResult, VarianceReducedResult, monte_carlo,
                         monte_carlo_greeks)
from .american import AmericanMonteCarloResult, american_monte_carlo
from .greeks import Greeks, greeks
from .greeks_full import FullGreeks, LocalVolSurface, greeks_full, local_vol
from .param_sens import ParameterSensitivities, parameter_sensitivities
from .ffn import FFNModel, fine_tune_ffn, price_features, train_ffn, train_ffn_on_generator
from ._native import NativeError

__all__ = ["DoubleHeston", "DoubleHestonJumpCalibrator", "CalibrationResult",
           "generate_synthetic_calibrations", "implied_vol", "NativeError", "calibrate_batch",
           "BatchCalibrationResult", "monte_carlo", "MonteCarloResult",
           "VarianceReducedResult", "monte_carlo_greeks", "MonteCarloGreeks",
           "american_monte_carlo", "AmericanMonteCarloResult", "greeks", "Greeks",
           "greeks_full", "FullGreeks", "local_vol", "LocalVolSurface",
           "parameter_sensitivities", "ParameterSensitivities", "ParameterUncertainty",
           "FFNModel", "train_ffn", "train_ffn_on_generator", "fine_tune_ffn", "price_features"]
__version__ = "0.1.0"
