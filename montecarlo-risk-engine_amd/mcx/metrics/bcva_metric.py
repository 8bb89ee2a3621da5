"""Bilateral CVA: CVA, DVA and their first-to-default forms from one pass over the unsecured exposures.

With c the counterparty, o the own name, x_k the netting set's unsecured exposure at metric date t_k (signed, discounted),
S_n(k) = S_n(0, t_k), q_n(k) = 1 - S_n(t_k, t_{k+1}) and the sums over k = 0 .. E-2, per path:

    cva     = (1-R_c) sum relu( x_k) S_c(k) q_c(k)              (CVAMetric)
    dva     = (1-R_o) sum relu(-x_k) S_o(k) q_o(k)
    cva_ftd = (1-R_c) sum relu( x_k) S_c(k) q_c(k) S_o(k)
    dva_ftd = (1-R_o) sum relu(-x_k) S_o(k) q_o(k) S_c(k)
    bcva    = cva_ftd - dva_ftd                                 (per path; positive = cost)

Each evaluation is (mean, std(unbiased)/sqrt(N)) over the paths.  On the HIP backend the five come from one kernel
(csrc/k4_xva.hip, mcx_reduce_xva) through atoms; `evaluate_numerically` is the same table in torch from `exposures` and
`resolved_requests`, for a backend without reduce_xva."""
from collections import defaultdict

import torch

from ..request_interface.request_types import AtomicRequest, AtomicRequestType
from .metric import Metric, MetricType


def survival_requests(exposure_timeline, name: str):
    """the two requests per date CVAMetric registers (cva_metric.py:23-46), for `name`: ({label: S(0,t_k)}, {label: S(t_k,t_k+1)})
    with label = (k, name)"""
    surv, cond = {}, {}
    for idx in range(len(exposure_timeline) - 1):
        label = (idx, name)
        cond[label] = AtomicRequest(AtomicRequestType.CONDITIONAL_SURVIVAL_PROBABILITY,
                                    time1=exposure_timeline[idx], time2=exposure_timeline[idx + 1])
        surv[label] = AtomicRequest(AtomicRequestType.SURVIVAL_PROBABILITY)
    return surv, cond


def _resolved(resolved_requests, req, who: str):
    if req.handle is None:
        raise ValueError(f"{who}: a survival request has no handle. Equal requests of two metrics on one name are de-duplicated and "
                         "only one of them receives its handle, so on a backend without reduce_xva this metric cannot share a name "
                         "with another CVA / DVA / bilateral CVA metric of the same RiskMetrics (the HIP backend has no such limit)")
    return resolved_requests[0][req.handle]


def xva_integrands(exposures, resolved_requests, cp, own, who: str):
    """per-path (cva, dva, cva_ftd, dva_ftd, bcva) by the table.  cp / own: (name, recovery, surv requests, cond requests) or
    None for a party that never defaults (S = 1, q = 0)"""
    acc = [torch.zeros_like(exposures[0]) for _ in range(4)]
    for k in range(len(exposures) - 1):
        S, q = [], []
        for side in (cp, own):
            if side is None:
                S.append(1.0); q.append(0.0)
            else:
                label = (k, side[0])
                S.append(_resolved(resolved_requests, side[2][label], who))
                q.append(1.0 - _resolved(resolved_requests, side[3][label], who))
        ep, en = torch.relu(exposures[k]), torch.relu(-exposures[k])
        wc, wo = S[0] * q[0], S[1] * q[1]
        acc[0] = acc[0] + ep * wc
        acc[1] = acc[1] + en * wo
        acc[2] = acc[2] + ep * (wc * S[1])
        acc[3] = acc[3] + en * (wo * S[0])
    lc = 1.0 - cp[1] if cp is not None else 1.0
    lo = 1.0 - own[1] if own is not None else 1.0
    cva, dva, cftd, dftd = acc[0] * lc, acc[1] * lo, acc[2] * lc, acc[3] * lo
    return cva, dva, cftd, dftd, cftd - dftd


class BilateralCVAMetric(Metric):
    _native = True
    EVALUATIONS = ("cva", "dva", "cva_ftd", "dva_ftd", "bcva")

    def __init__(self, counterparty_id: str, own_id: str, recovery_rate: float, own_recovery_rate: float,
                 evaluation_type=Metric.EvaluationType.NUMERICAL):
        super().__init__(MetricType.BCVA, evaluation_type)
        if counterparty_id == own_id:
            raise ValueError("BilateralCVAMetric: the counterparty and the own name must differ")
        self.counterparty_id = counterparty_id
        self.own_id = own_id
        self.recovery_rate = recovery_rate
        self.own_recovery_rate = own_recovery_rate
        self.survival_prob_requests: dict = {}
        self.cond_survival_prob_requests: dict = {}
        self.own_survival_prob_requests: dict = {}
        self.own_cond_survival_prob_requests: dict = {}

    def get_counterparty_ids(self):
        return [self.counterparty_id, self.own_id]

    def get_name(self) -> str:
        return f"bcva[{self.counterparty_id}|{self.own_id}]"

    def set_requests(self, exposure_timeline) -> None:
        self.survival_prob_requests, self.cond_survival_prob_requests = survival_requests(exposure_timeline, self.counterparty_id)
        self.own_survival_prob_requests, self.own_cond_survival_prob_requests = survival_requests(exposure_timeline, self.own_id)

    def get_requests(self):
        out = defaultdict(list)
        for table in (self.survival_prob_requests, self.cond_survival_prob_requests,
                      self.own_survival_prob_requests, self.own_cond_survival_prob_requests):
            for label, req in table.items():
                out[label].append(req)
        return out

    def evaluate_numerically(self, exposures, resolved_requests, **kwargs):
        cp = (self.counterparty_id, self.recovery_rate, self.survival_prob_requests, self.cond_survival_prob_requests)
        own = (self.own_id, self.own_recovery_rate, self.own_survival_prob_requests, self.own_cond_survival_prob_requests)
        return [self._compute_mc_mean_and_error(v) for v in xva_integrands(exposures, resolved_requests, cp, own, self.get_name())]
