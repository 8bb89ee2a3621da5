"""The numpy restatement of the storage's dynamic programme (tests/storage_reference.py) against the reference's fixtures: fed
with the fixtures' paths it must give the fixtures' coefficients, cashflows and exposures — WITH the float32 step buffer of the
reference, and visibly not without it.  It is then the checker of GPU runs on Philox paths (tests/test_storage_gpu.py).

Bounds: coefficients 1e-9 of the largest coefficient of the date's [S][K] block (two least-squares solvers on raw monomials);
cashflows and exposures 1e-12 of the largest entry (the same float64 formulas, summed in another order)."""
import numpy as np
import pytest

import storage_cases
from storage_reference import AtomReader, StorageRestatement


def compiled_controller(name):
    """host-side compilation only (atoms, coefficient layout): no backend is touched"""
    from mcx.plan import BookPlan
    from oracle_backend import OracleBackend
    sc, g = storage_cases.make_controller(name, OracleBackend(), inject=False)
    sc._compile()
    sc._register_regression_atoms()
    sc.book_plan = BookPlan(sc._comp, *sc._plan_args)
    return sc, storage_cases.load_golden(name)


def restate(sc, g, p_i, float32_quirk=True):
    p = sc.products[p_i]
    K = sc.regression_function.get_degree()
    asset = p.asset_ids[0]
    pre = AtomReader(sc, np.transpose(g["paths_pre"], (1, 2, 0)))
    main = AtomReader(sc, np.transpose(g["paths_main"], (1, 2, 0)))
    rs = StorageRestatement(p, K, float32_quirk)
    expo_times = [float(t) for t in sc.exposure_timeline]
    back = rs.backward(expo_times, lambda t: pre.spot(asset, t), pre.numeraire)
    prod_coeffs = np.stack([back[t]["coeffs"] for t in rs.dates])
    expo_coeffs = np.stack([back[t]["coeffs"] if t in back else np.zeros((rs.S, K)) for t in expo_times])
    cfs, expo, margin = rs.forward(expo_times, True, lambda t: main.spot(asset, t), main.numeraire, prod_coeffs, expo_coeffs)
    return dict(prod_coeffs=prod_coeffs, expo_coeffs=expo_coeffs, cfs=cfs, expo=expo, margin=margin)


def storages_of(sc):
    return [i for i, p in enumerate(sc.products) if getattr(p, "is_storage", False)]


@pytest.mark.parametrize("name", list(storage_cases.CASES))
def test_restatement_reproduces_the_fixture_with_the_float32_quirk(name):
    sc, g = compiled_controller(name)
    for p_i in storages_of(sc):
        r = restate(sc, g, p_i)
        for key, ours in (("prod_coeffs", r["prod_coeffs"]), ("expo_coeffs", r["expo_coeffs"])):
            ref = g[f"{key}_{p_i}"]
            for d in range(len(ref)):
                big = np.abs(ref[d]).max()
                err = np.abs(ours[d] - ref[d]).max()
                print(name, p_i, key, d, "coefficient error / largest", err / max(big, 1e-300))
                assert err <= 1e-9 * big, (name, p_i, key, d, err, big)
        for key, ours in (("cfs", r["cfs"]), ("exposures", r["expo"])):
            ref = g[f"{key}_{p_i}"]
            err, big = np.abs(ours - ref).max(), np.abs(ref).max()
            print(name, p_i, key, "error / largest", err / big)
            assert err <= 1e-12 * big, (name, p_i, key, err, big)
        assert r["margin"].min() >= 1e-9          # (the generator's min_rel_gap covers every decision, this one the realised ones)


@pytest.mark.parametrize("name", ["storage_const", "storage_shift"])
def test_restatement_without_the_quirk_differs_from_the_fixture(name):
    """a float64 step buffer moves the cached cashflows by ~1e-7 relative: far outside the bound above"""
    sc, g = compiled_controller(name)
    p_i = storages_of(sc)[0]
    r = restate(sc, g, p_i, float32_quirk=False)
    ref = g[f"prod_coeffs_{p_i}"]
    rel = max(np.abs(r["prod_coeffs"][d] - ref[d]).max() / np.abs(ref[d]).max() for d in range(len(ref) - 1))
    assert rel > 1e-8, rel


@pytest.mark.parametrize("name", list(storage_cases.CASES))
def test_fixture_robustness_numbers(name):
    """what makes 'no path may differ' a fair demand: no decision of the reference closer than 1e-9, no tie whose outcome
    depends on the tie-break, every action taken"""
    g = storage_cases.load_golden(name)
    assert float(g["min_rel_gap"]) >= 1e-9
    assert int(g["ties_with_different_outcome"]) == 0
    assert int(g["ties"]) > 0 and (g["actions_taken"] > 0).all()
