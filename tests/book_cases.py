"""Small purpose-made books for the kernel-level tests of K2 (tests/test_book_kernels.py, tests/test_book_reference.py).

Each is compiled by SimulationController.prepare() from the classes of tests/cases.py, with short schedules (a path costs at most
a few hundred atom evaluations), and covers one FEAT mask of mcx_eval_book's dispatch (csrc/k2_book.hip):
  plain        0                cashflows, a plain option, polynomial exposures, no `den` term
  den          DEN              + a swap with tenor_fixed != tenor_float
  exercise     DEN|EXERCISE     + a FlexiCall with 4 exercise states and a Bermudan put
  exotic       DEN|EX|EXOTIC    + geometric basket, control-variate basket, binary
  all          ALL              analytic Black-Scholes exposures (EXPO_BS, one with aux[2] == 0 at maturity) + exercise + exotic
  netting      DEN              two netting sets; two products write every exposure row of the first, with a product without
                                Monte-Carlo events (ev_begin == ev_end) spliced between them
  barrier      (scalar only)    discretely monitored barriers, mode 4 and mode 5 (Brownian bridge, injected uniforms)
  many         0                72 products: the product-chunked launch
`expo_only=True` drops the PV metric: want_cfs = 0, the cash events of stateless products are skipped.
After prepare() the regression's own coefficients are perturbed (perturbed_coeffs) so that no coefficient row is zero or equal to
another state's."""
import copy

import numpy as np

import cases
from mcx import _abi

K2F_DEN, K2F_EXOTIC, K2F_EXERCISE, K2F_BS_EXPO = _abi.K2F_DEN, _abi.K2F_EXOTIC, _abi.K2F_EXERCISE, _abi.K2F_BS_EXPO
FEAT = {"plain": 0, "den": K2F_DEN, "exercise": K2F_DEN | K2F_EXERCISE, "exotic": K2F_DEN | K2F_EXERCISE | K2F_EXOTIC,
        "all": 15, "netting": K2F_DEN, "many": 0}
N_PRE = 2048
COEFF_SEED = 0           # (chosen so that every exercise state of the FlexiCall and of the Bermudan ends populated: test_book_reference.py)


def _metrics(expo_only, tl, pfe=False):
    mets = [cases.EPEMetric()] + ([cases.PFEMetric(0.9)] if pfe else []) + ([] if expo_only else [cases.PVMetric()])
    return cases.RiskMetrics(mets, exposure_timeline=np.asarray(tl, dtype=float))


def _vasicek():
    return cases.VasicekModel(0.0, 0.02, 0.04, 0.3, 0.015, asset_id="r")


def _named(p, name):
    p.name = name
    return p


def _rates_products(den):
    P = [_named(cases.Bond(0.0, 1.0, 1.0, 0.5, True, 0.03, "r"), "bond"),
         _named(cases.InterestRateSwap(0.0, 1.0, 2.0, 0.035, 0.25, 0.25, cases.IRSType.RECEIVER, "r"), "swap_eq"),
         _named(cases.EuropeanOption(cases.Bond(0.0, 1.5, 1.0, 0.5, True, 0.04, "r"), 0.75, 0.98, cases.OptionType.CALL, asset_id="r"), "bond_call")]
    if den:
        P.append(_named(cases.InterestRateSwap(0.0, 1.0, 1.0, 0.025, 0.5, 0.25, cases.IRSType.PAYER, "r"), "swap_uneq"))
    return P


def plain(expo_only=False):
    return [cases.NettingSet(name="ns", products=_rates_products(False))], _vasicek(), _metrics(expo_only, [0.0, 0.25, 0.5, 0.75, 1.0]), 2, cases.A


def den(expo_only=False):
    return [cases.NettingSet(name="ns", products=_rates_products(True))], _vasicek(), _metrics(expo_only, [0.0, 0.25, 0.5, 0.75, 1.0]), 2, cases.A


def _eq_rates_model(n_eq):
    """n_eq Black-Scholes assets eq0.. (one BlackScholesMulti) + a Vasicek short rate "r\""""
    ids = [f"eq{k}" for k in range(n_eq)]
    corr = np.full((n_eq, n_eq), 0.3)
    np.fill_diagonal(corr, 1.0)
    market = cases.BlackScholesMulti(0.0, 0.03, ids, [100.0 + 5.0 * k for k in range(n_eq)], [0.25 - 0.03 * k for k in range(n_eq)], corr)
    rates = cases.VasicekModel(0.0, 0.02, 0.04, 0.3, 0.015, asset_id="r")
    return ids, cases.ModelConfig([market, rates], inter_asset_correlation_matrix=[np.full((n_eq, 1), 0.1)])


def _exercise_products(a):
    opts = [cases.EuropeanOption(cases.Equity(a), 0.2 * (k + 1), 97.0 + 1.5 * k, cases.OptionType.PUT, asset_id=a) for k in range(5)]
    return [_named(cases.FlexiCall(opts, 3, asset_id=a), "flexi"),                           # 4 exercise states
            _named(cases.BermudanOption(cases.Equity(a), [0.2, 0.4, 0.6, 0.8, 1.0], 100.0, cases.OptionType.PUT, asset_id=a), "bermudan")]


class _ControlVariateBasket(cases.BasketOption):
    """the basket with its geometric control variate inside a ModelConfig: the analytic correction term (aux[1]) comes from the
    equity sub-model (BasketOption asks the model itself, which only a stand-alone BlackScholesMulti answers)"""

    def compute_pv_analytically(self, model):
        return super().compute_pv_analytically(model.models[0] if isinstance(model, cases.ModelConfig) else model)


def _exotic_products(ids):
    return [_named(cases.BasketOption(0.6, ids[:2], [0.6, 0.4], 100.0, cases.OptionType.PUT, cases.BasketOptionType.GEOMETRIC), "geo"),
            _named(_ControlVariateBasket(0.8, ids[:2], [0.5, 0.5], 101.0, cases.OptionType.CALL, cases.BasketOptionType.ARITHMETIC, True), "cv"),
            _named(cases.BinaryOption(0.4, 100.5, 10.0, cases.OptionType.CALL, asset_id=ids[0]), "binary_call"),
            _named(cases.BinaryOption(1.0, 99.0, 5.0, cases.OptionType.PUT, asset_id=ids[0]), "binary_put")]


_TL_EQ = [0.0, 0.2, 0.4, 0.6, 0.8, 1.0]


def exercise(expo_only=False):
    ids, model = _eq_rates_model(1)
    P = [_named(cases.InterestRateSwap(0.0, 0.8, 50.0, 0.025, 0.4, 0.2, cases.IRSType.PAYER, "r"), "swap_uneq")] + _exercise_products(ids[0])
    return [cases.NettingSet(name="ns", products=P)], model, _metrics(expo_only, _TL_EQ), 1, cases.E


def exotic(expo_only=False):
    ids, model = _eq_rates_model(2)
    P = ([_named(cases.InterestRateSwap(0.0, 0.8, 50.0, 0.025, 0.4, 0.2, cases.IRSType.PAYER, "r"), "swap_uneq")]
         + _exercise_products(ids[0]) + _exotic_products(ids))
    return [cases.NettingSet(name="ns", products=P)], model, _metrics(expo_only, _TL_EQ), 1, cases.E


def all_(expo_only=False):
    ids = ["eq0", "eq1"]
    model = cases.BlackScholesMulti(0.0, 0.03, ids, [100.0, 105.0], [0.25, 0.22], np.array([[1.0, 0.3], [0.3, 1.0]]))
    P = ([_named(cases.EuropeanOption(cases.Equity(ids[0]), 0.8, 95.0, cases.OptionType.CALL, asset_id=ids[0]), "call"),     # tau = 0 at row 0.8
          _named(cases.EuropeanOption(cases.Equity(ids[1]), 1.0, 110.0, cases.OptionType.PUT, asset_id=ids[1]), "put")]
         + _exercise_products(ids[0]) + _exotic_products(ids))
    return [cases.NettingSet(name="ns", products=P)], model, _metrics(expo_only, _TL_EQ, pfe=True), 1, cases.A


def netting(expo_only=False):
    ns1 = cases.NettingSet(name="ns1", products=[_named(cases.InterestRateSwap(0.0, 1.0, 1.0, 0.025, 0.5, 0.25, cases.IRSType.PAYER, "r"), "swap_uneq"),
                                                  _named(cases.Bond(0.0, 1.0, 1.0, 0.5, True, 0.03, "r"), "bond")], threshold=0.002)
    ns2 = cases.NettingSet(name="ns2", products=[_named(cases.Bond(0.0, 0.75, 0.5, 0.25, True, None, "r"), "frn")])
    return [ns1, ns2], _vasicek(), _metrics(expo_only, [0.0, 0.25, 0.5, 0.75, 1.0]), 2, cases.A


def barrier(expo_only=False):
    assert not expo_only
    model = cases.BlackScholesModel(0, 100.0, 0.03, 0.25)
    B = cases.BarrierOptionType
    prods = [cases.BarrierOption(0.0, 1.0, 100.0, 4, cases.OptionType.CALL, 125.0, B.UPANDOUT),
             cases.BarrierOption(0.0, 1.0, 95.0, 4, cases.OptionType.CALL, 85.0, B.DOWNANDOUT, 130.0, B.UPANDOUT),
             cases.BarrierOption(0.0, 1.0, 105.0, 4, cases.OptionType.PUT, 90.0, B.DOWNANDIN)]
    for k, p in enumerate(prods):
        p.name = f"b{k}"
    prods[1].set_use_brownian_bridge()
    prods[2].set_use_brownian_bridge()
    return [cases.NettingSet(name=p.name, products=[p]) for p in prods], model, cases.RiskMetrics([cases.PVMetric()]), 1, cases.A


N_MANY = 72


def many(expo_only=False):
    P = []
    for k in range(N_MANY):
        if k % 3 == 0:
            p = cases.Bond(0.0, 0.5 + 0.25 * (k % 3), 1.0 + 0.01 * k, 0.25, True, 0.02 + 0.0005 * k, "r")
        elif k % 3 == 1:
            p = cases.InterestRateSwap(0.0, 0.75, 1.0 + 0.02 * k, 0.02 + 0.0003 * k, 0.25, 0.25, cases.IRSType.PAYER if k % 2 else cases.IRSType.RECEIVER, "r")
        else:
            p = cases.Bond(0.0, 0.5, 0.5 + 0.01 * k, 0.25, True, None, "r")
        P.append(_named(p, f"p{k}"))
    return [cases.NettingSet(name="a", products=P[:40]), cases.NettingSet(name="b", products=P[40:])], _vasicek(), \
        _metrics(expo_only, [0.0, 0.25, 0.5, 0.75]), 1, cases.A


BUILDERS = {"plain": plain, "den": den, "exercise": exercise, "exotic": exotic, "all": all_, "netting": netting, "barrier": barrier,
            "many": many}
EXPO_ONLY = ("plain", "den", "exercise", "netting", "many")          # books that also come in a want_cfs = 0 variant
REFERENCE_BOOKS = [(b, False) for b in BUILDERS if b != "barrier"] + [(b, True) for b in EXPO_ONLY]


def perturbed_coeffs(sc, coeffs, seed=COEFF_SEED):
    """the regression's own coefficients, perturbed so that no row is zero or equal to another state's — in the spirit of
    test_lsm_basis_sizes._Ctx, but row by row: a row [K] is scaled as a whole by 1 + 0.05 N (its monomials keep cancelling as the
    regression left them, so the exercise decisions stay path-dependent; independent noise of 0.01 on the x^2 coefficient of an
    equity at x ~ 100 would decide every path the same way), every coefficient then by 1 + 1e-3 N, and a zero row (state 0, dates
    past maturity) becomes 0.01 N times the product's mean row.  Constants parked behind a product's blocks (the bridge
    parameters) are left alone."""
    out = np.array(coeffs, dtype=np.float64)
    r = np.random.default_rng(seed)
    K = sc.book_plan.n_basis
    for p_i, p in enumerate(sc.products):
        S = p.get_num_states()
        blk = out[sc._expo_coeff_base[p_i]:sc._extra_coeff_base[p_i]].reshape(-1, S, K)          # (a view)
        nz = np.abs(blk).sum(axis=2) > 0
        tmpl = blk[nz].mean(axis=0) if nz.any() else np.ones(K)
        blk *= (1.0 + 0.05 * r.standard_normal(blk.shape[:2]))[..., None]
        blk *= 1.0 + 1e-3 * r.standard_normal(blk.shape)
        blk[~nz] = 0.01 * r.standard_normal(int((~nz).sum()))[:, None] * tmpl
    return out


def with_empty_product(plan, after, netting_set):
    """a copy of the plan with a product without Monte-Carlo events (an analytically valued one: ev_begin == ev_end) inserted after
    product `after`"""
    q = copy.copy(plan)
    row = np.zeros(1, dtype=_abi.PRODUCT_DTYPE)
    row["netting_set"], row["n_states"] = netting_set, 1
    q.products = np.ascontiguousarray(np.concatenate([plan.products[:after + 1], row, plan.products[after + 1:]]))
    q.coeffs = plan.coeffs.copy()
    d = _abi.BookDesc()
    for name, _t in _abi.BookDesc._fields_:
        setattr(d, name, getattr(plan.desc, name))
    d.n_products = len(q.products)
    d.products, d.coeffs = _abi.ptr(q.products), _abi.ptr(q.coeffs)
    q.desc = d
    return q


class Book:
    """one compiled book on `backend`: controller, plan (coefficients perturbed, shared with an oracle book when asked) and book"""

    def __init__(self, name, backend, expo_only=False):
        ns, model, rm, steps, scheme = BUILDERS[name](expo_only)
        self.name, self.expo_only = name, expo_only
        sc = cases.SimulationController(ns, model, rm, 1024, N_PRE, steps, scheme, backend=backend)
        sc.allow_fused = False
        sc.prepare()
        self.sc, self.plan, self.book = sc, sc.book_plan, sc.book
        if name == "netting":
            self.plan = with_empty_product(sc.book_plan, 0, 1)
            self.book = backend.book_create(self.plan)
        self.base_coeffs = self.plan.coeffs.copy()
        self.set_coeffs(backend, perturbed_coeffs(sc, self.base_coeffs))
        assert bool(self.plan.desc.want_cfs) == (not expo_only) and (name == "barrier" or self.plan.desc.want_expo)

    def set_coeffs(self, backend, c):
        backend.book_set_coeffs(self.book, 0, c)           # (writes plan.coeffs too: the oracle and the reference read that array)
        assert np.array_equal(self.plan.coeffs, c)

    def used_rows(self):
        """(date, state) rows of the paths tensor some atom names"""
        a = self.plan.atoms
        return {(int(t), int(c)) for t, c in zip(a["t_idx"], a["col"]) if c >= 0}
