"""FVA: the funding cost and the funding benefit of a netting set's unsecured exposure, from one pass over the exposures.

With c the counterparty, o the own name, x_k the netting set's unsecured exposure at metric date t_k (signed, discounted, after
threshold, MPoR and collateral) and the sums over k = 0 .. E-2, per path:

    w(k)     = S_c(0,t_k) S_o(0,t_k)                            (a name that is None never defaults: its S is 1)
    phi_b(k) = 1 - exp(-int_{t_k}^{t_k+1} s_b(u) du)            borrowing weight
    phi_l(k) = 1 - exp(-int_{t_k}^{t_k+1} s_l(u) du)            lending weight
    fca      = sum relu( x_k) w(k) phi_b(k)                     funding cost adjustment
    fba      = sum relu(-x_k) w(k) phi_l(k)                     funding benefit adjustment
    fva      = fca - fba                                        (per path; positive = cost)

A left-point rule on the metric timeline, like CVA here.  s_b and s_l are deterministic funding spreads: a float (flat) or a dict
{tenor: spread} read as CIRPPModel._lambda_market reads its hazard rates, s(u) = s_i for t_{i-1} < u <= t_i and the last value beyond
the last tenor; the integral is exact over the segments and phi is -expm1(-I) in float64 on the host (`funding_weights`).

Each evaluation is (mean, std(unbiased)/sqrt(N)) over the paths.  On the HIP backend the three come from one kernel (csrc/k4_fva.hip,
mcx_reduce_fva) through atoms; `evaluate_numerically` is the same table in torch from `exposures` and `resolved_requests`, for a
backend without reduce_fva.  It keeps the limitation of the host forms: equal requests of two metrics on one name are de-duplicated,
so there the metric cannot share a name with another xVA metric of the same RiskMetrics (`bcva_metric._resolved` raises).

The metric type is `XvaMetricType.FVA`, a member of a second enum: `MetricType` keeps its member set, and every dispatch on
`metric.metric_type` compares members or tests membership, so this type falls through every branch written for the first enum
(mcx/metrics/metric.py).  The counterparty gates the metric as it gates CVAMetric (a netting set of another counterparty gets zeros;
None applies to every set); the own name never gates.  With a name the run needs a ModelConfig holding that name's model, as DVA
does; with no names the metric runs under any model."""
import math
from collections import defaultdict

import torch

from ..request_interface.request_types import AtomicRequest, AtomicRequestType
from .bcva_metric import _resolved
from .metric import Metric, XvaMetricType


def _check_spread(spread, what: str):
    """-> ([tenors], [values]) of the piecewise-constant curve; a flat spread is ([], [value])"""
    if isinstance(spread, dict):
        if not spread:
            raise ValueError(f"FVAMetric: the {what} spread curve is empty")
        tenors, values = [float(t) for t in spread.keys()], [float(v) for v in spread.values()]
        if any(not math.isfinite(t) for t in tenors) or any(b <= a for a, b in zip(tenors, tenors[1:])):
            raise ValueError(f"FVAMetric: the tenors of the {what} spread curve must be finite and increasing")
    else:
        tenors, values = [], [float(spread)]
    if any(not math.isfinite(v) for v in values):
        raise ValueError(f"FVAMetric: the {what} spread is not finite")
    return tenors, values


def spread_integral(spread, t0: float, t1: float) -> float:
    """int_{t0}^{t1} s(u) du of the piecewise-constant curve, exact over its segments (t0 <= t1)"""
    tenors, values = _check_spread(spread, "funding")
    total, lo = 0.0, float(t0)
    for tenor, value in zip(tenors, values):
        hi = min(float(t1), tenor)
        if hi > lo:
            total += value * (hi - lo)
            lo = hi
    if float(t1) > lo:
        total += values[-1] * (float(t1) - lo)
    return total


def funding_weights(spread, timeline) -> list:
    """phi(k) = 1 - exp(-int_{t_k}^{t_k+1} s(u) du) for the E-1 intervals of `timeline`, float64"""
    t = [float(x) for x in timeline]
    return [-math.expm1(-spread_integral(spread, t[k], t[k + 1])) for k in range(len(t) - 1)]


def survival_only_requests(exposure_timeline, name: str):
    """{(k, name): S(0,t_k)} for the E-1 left points: the unconditional half of bcva_metric.survival_requests"""
    return {(idx, name): AtomicRequest(AtomicRequestType.SURVIVAL_PROBABILITY) for idx in range(len(exposure_timeline) - 1)}


def fva_integrands(exposures, resolved_requests, cp, own, w_borrow, w_lend, who: str):
    """per-path (fca, fba, fva) by the table.  cp / own: (name, surv requests) or None for a party that never defaults"""
    fca, fba = torch.zeros_like(exposures[0]), torch.zeros_like(exposures[0])
    for k in range(len(exposures) - 1):
        S = [1.0 if side is None else _resolved(resolved_requests, side[1][(k, side[0])], who) for side in (cp, own)]
        w = S[0] * S[1]
        fca = fca + torch.relu(exposures[k]) * (w * w_borrow[k])
        fba = fba + torch.relu(-exposures[k]) * (w * w_lend[k])
    return fca, fba, fca - fba


class FVAMetric(Metric):
    _native = True
    EVALUATIONS = ("fca", "fba", "fva")

    def __init__(self, borrow_spread, lend_spread=None, counterparty_id=None, own_id=None,
                 evaluation_type=Metric.EvaluationType.NUMERICAL):
        super().__init__(XvaMetricType.FVA, evaluation_type)
        if lend_spread is None:
            lend_spread = borrow_spread
        _check_spread(borrow_spread, "borrowing")
        _check_spread(lend_spread, "lending")
        if counterparty_id is not None and counterparty_id == own_id:
            raise ValueError("FVAMetric: the counterparty and the own name must differ")
        self.borrow_spread = borrow_spread
        self.lend_spread = lend_spread
        self.counterparty_id = counterparty_id
        self.own_id = own_id
        self.survival_prob_requests: dict = {}
        self.own_survival_prob_requests: dict = {}
        self.w_borrow: list = []
        self.w_lend: list = []

    def get_counterparty_ids(self):
        return [name for name in (self.counterparty_id, self.own_id) if name is not None]

    def get_name(self) -> str:
        if self.counterparty_id is None and self.own_id is None:
            return "fva"
        return f"fva[{self.counterparty_id or ''}|{self.own_id or ''}]"

    def set_requests(self, exposure_timeline) -> None:
        self.survival_prob_requests = {} if self.counterparty_id is None else survival_only_requests(exposure_timeline, self.counterparty_id)
        self.own_survival_prob_requests = {} if self.own_id is None else survival_only_requests(exposure_timeline, self.own_id)
        self.w_borrow = funding_weights(self.borrow_spread, exposure_timeline)
        self.w_lend = funding_weights(self.lend_spread, exposure_timeline)

    def get_requests(self):
        out = defaultdict(list)
        for table in (self.survival_prob_requests, self.own_survival_prob_requests):
            for label, req in table.items():
                out[label].append(req)
        return out

    def evaluate_numerically(self, exposures, resolved_requests, **kwargs):
        if len(exposures) < 2:                   # one metric date: no interval, three exact zeros
            return [(0.0, 0.0) for _ in self.EVALUATIONS]
        cp = None if self.counterparty_id is None else (self.counterparty_id, self.survival_prob_requests)
        own = None if self.own_id is None else (self.own_id, self.own_survival_prob_requests)
        return [self._compute_mc_mean_and_error(v)
                for v in fva_integrands(exposures, resolved_requests, cp, own, self.w_borrow, self.w_lend, self.get_name())]
