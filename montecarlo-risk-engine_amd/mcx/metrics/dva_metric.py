"""DVA = (1-R_o) * E[ sum_k relu(-E_k) S_o(0,t_k) (1 - S_o(t_k,t_{k+1})) ]: the CVA formula on the negative part of the exposure
with the survival of the own name.  On the HIP backend it is the `dva` record of mcx_reduce_xva (csrc/k4_xva.hip) with no
counterparty; `evaluate_numerically` is the host form (bcva_metric.xva_integrands).  Applies to every netting set."""
from collections import defaultdict

from .bcva_metric import survival_requests, xva_integrands
from .metric import Metric, MetricType


class DVAMetric(Metric):
    _native = True

    def __init__(self, own_id: str, recovery_rate: float, evaluation_type=Metric.EvaluationType.NUMERICAL):
        super().__init__(MetricType.DVA, evaluation_type)
        self.own_id = own_id
        self.recovery_rate = recovery_rate
        self.survival_prob_requests: dict = {}
        self.cond_survival_prob_requests: dict = {}

    def get_counterparty_ids(self):
        return [self.own_id]

    def get_name(self) -> str:
        return f"dva[{self.own_id}]"

    def set_requests(self, exposure_timeline) -> None:
        self.survival_prob_requests, self.cond_survival_prob_requests = survival_requests(exposure_timeline, self.own_id)

    def get_requests(self):
        out = defaultdict(list)
        for table in (self.survival_prob_requests, self.cond_survival_prob_requests):
            for label, req in table.items():
                out[label].append(req)
        return out

    def evaluate_numerically(self, exposures, resolved_requests, **kwargs):
        own = (self.own_id, self.recovery_rate, self.survival_prob_requests, self.cond_survival_prob_requests)
        return [self._compute_mc_mean_and_error(xva_integrands(exposures, resolved_requests, None, own, self.get_name())[1])]
