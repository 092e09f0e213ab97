"""Analytic sensitivities of the COS price to the thirteen model parameters
(dh_surface_param_sens, csrc/dh_param_grad.h).

``parameter_sensitivities`` takes the parameters a calibration returns and a list of the
reference's option dicts and returns, from one pass on the GPU, the price and its partial
derivative with respect to every model parameter: the two initial variances (the Greeks' vegas),
and kappa, theta, sigma, rho of each factor and the three jump parameters, which otherwise cost a
bump and a repricing each.

What is differentiated: the reference's COS series (double_heston.py:160-192) at a FIXED
truncation range ``[a, b]``, as ``dhcos.greeks`` does: not through the cumulant range or its
``log(K / S0) -+ 0.1`` clamp.  Where the clamp is inactive the difference from a bump-and-reprice
quotient is of the size of the quotient's own error.  The derivatives are with respect to the model
parameters themselves (``sigma1``, not its logarithm).

Every argument the native library refuses is refused here first, with ``ValueError`` and before
the library is loaded.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import _native
from .greeks import _options, _records, check_L


@dataclass
class ParameterSensitivities:
    """The fourteen planes of one request: scalars (``DoubleHeston.parameter_sensitivities``),
    ``[M]`` for one parameter set or ``[P, M]`` for ``P`` (``dhcos.parameter_sensitivities``).
    ``price`` is the COS price; every other field is d price / d (that model parameter) at a fixed
    truncation range (see the module docstring)."""
    price: np.ndarray
    v1_0: np.ndarray
    kappa1: np.ndarray
    theta1: np.ndarray
    sigma1: np.ndarray
    rho1: np.ndarray
    v2_0: np.ndarray
    kappa2: np.ndarray
    theta2: np.ndarray
    sigma2: np.ndarray
    rho2: np.ndarray
    lambda_j: np.ndarray
    mu_j: np.ndarray
    sigma_j: np.ndarray

    @classmethod
    def from_planes(cls, planes):
        """planes[i] in _native.PARAM_SENS' order -> ParameterSensitivities."""
        return cls(*(planes[i] for i in range(len(_native.PARAM_SENS))))


def check_N(N):
    if int(N) != N or not 1 <= N <= _native.PARAM_GRAD_MAX_N:
        raise ValueError(f"N: a whole number in [1, {_native.PARAM_GRAD_MAX_N}], got {N!r}")
    return int(N)


def parameter_sensitivities(parameters, spot, risk_free, options, N=128, q=0.0, L=10.0,
                            device=None) -> ParameterSensitivities:
    """Price and its analytic sensitivity to each of the 13 model parameters, for ``options``
    under every parameter set, on the GPU.

    parameters: a dict of the 13 names, a ``[13]`` array or ``[P, 13]``; spot, risk_free, q:
    scalars or ``[P]``; options: the reference's list of dicts (``strike``, ``maturity``,
    ``option_type``).  Returns ``ParameterSensitivities`` of ``[M]`` arrays for one set,
    ``[P, M]`` for ``P``, in the options' order.  ``1 <= N <= 1024``.

    Partial derivatives of the COS series with ``N`` terms at a fixed truncation range (width
    ``L``): not through the cumulant range or its log-strike clamp (the module docstring).  The
    same call gives the same bits."""
    N, L = check_N(N), check_L(L)
    rec, single = _records(parameters, spot, risk_free, q)
    K, T, call = _options(options)
    ctx = _native.default_context(device)
    surf = _native.Surface(ctx, K, T, call)
    try:
        planes = surf.param_sens(rec, N, L)
    finally:
        surf.close()
    return ParameterSensitivities.from_planes(planes[:, 0] if single else planes)


__all__ = ["ParameterSensitivities", "parameter_sensitivities"]
