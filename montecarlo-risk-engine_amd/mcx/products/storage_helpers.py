"""StorageConfig — the contract data of a gas storage (reference surface: products/storage_helpers.py).

Volume windows, volume-dependent injection / withdrawal rate curves and dated variable costs, plus the window optimiser that
tightens the configured windows date by date until every grid point of a date can reach the window of the next one.  All of it
is host arithmetic in Python floats, in the reference's operation order: the optimised windows are the base of every number
the kernels (csrc/k6_storage.hip) produce, so they must come out bit for bit the same."""
from __future__ import annotations

import math
from bisect import bisect_left, bisect_right
from dataclasses import dataclass, field

import torch

DATE_TOL = 1e-12
VOLUME_TOL = 1e-12


@dataclass(order=True)
class _RatePoint:
    point: float
    rate: float


@dataclass(order=True)
class _DatedCost:
    date: float
    cost: float


def _in_window(start: float, end: float, date: float) -> bool:
    """half-open [start, end) up to DATE_TOL; a window of zero length holds its own date"""
    if math.isclose(start, end, abs_tol=DATE_TOL):
        return math.isclose(start, date, abs_tol=DATE_TOL)
    return start - DATE_TOL <= date < end - DATE_TOL


@dataclass
class _RateSchedule:
    start_date: float
    end_date: float
    values: list = field(default_factory=list)

    def contains(self, date: float) -> bool:
        return _in_window(self.start_date, self.end_date, date)


@dataclass
class _VolumeWindow:
    start_date: float
    end_date: float
    vmin: float
    vmax: float
    penalty: float = 0.0          # stored, never read (as in the reference)

    def contains(self, date: float) -> bool:
        return _in_window(self.start_date, self.end_date, date)


def _covering(date: float, items: list, what: str):
    """the first window / schedule holding `date`; a date outside all of them takes the LAST one"""
    for it in items:
        if it.contains(date):
            return it
    if not items:
        raise ValueError(what)
    return items[-1]


class StorageConfig:
    _date_in_window = staticmethod(_in_window)

    @staticmethod
    def grid_step(vmin: float, vmax: float, num_states: int) -> float:
        """volume per unit of state; 0 for a window that is a single point"""
        if num_states <= 1 or math.isclose(vmin, vmax, abs_tol=VOLUME_TOL):
            return 0.0
        return (vmax - vmin) / (num_states - 1.0)

    @staticmethod
    def state_scale(vmin: float, vmax: float, num_states: int) -> float:
        """state per unit of volume; 0 for a window that is a single point"""
        if num_states <= 1 or math.isclose(vmin, vmax, abs_tol=VOLUME_TOL):
            return 0.0
        return (num_states - 1.0) / (vmax - vmin)

    @staticmethod
    def _interpolate_rate(point: float, rate_points: list) -> float:
        """piecewise-linear rate at one volume (Python floats): flat outside the knots"""
        if not rate_points:
            raise ValueError("Flexibility slice is empty.")
        if len(rate_points) == 1:
            return rate_points[0].rate
        xs = [p.point for p in rate_points]
        ys = [p.rate for p in rate_points]
        if point <= xs[0]:
            return ys[0]
        if point >= xs[-1]:
            return ys[-1]
        hi = bisect_right(xs, point)
        lo = hi - 1
        if math.isclose(xs[lo], xs[hi], abs_tol=VOLUME_TOL):
            return ys[hi]
        weight = (point - xs[lo]) / (xs[hi] - xs[lo])
        return ys[lo] + weight * (ys[hi] - ys[lo])

    @staticmethod
    def interpolate_rate_tensor(point: torch.Tensor, rate_points: list) -> torch.Tensor:
        """the same curve on a tensor of volumes.  Not the same arithmetic at a doubled knot: here the weight is 0 where two
        knots coincide under torch.isclose (the left rate), the scalar form returns the right one — both as in the reference;
        the device table (mcx_storage_date) follows this form, which is the one the simulation uses."""
        if not rate_points:
            raise ValueError("Flexibility slice is empty.")
        if len(rate_points) == 1:
            return torch.full_like(point, rate_points[0].rate)
        xp = point.new_tensor([p.point for p in rate_points])
        fp = point.new_tensor([p.rate for p in rate_points])
        left = torch.clamp(torch.bucketize(point, xp) - 1, min=0, max=len(rate_points) - 2)
        x0, x1, y0, y1 = xp[left], xp[left + 1], fp[left], fp[left + 1]
        w = torch.where(torch.isclose(x0, x1), torch.zeros_like(point), (point - x0) / (x1 - x0))
        out = y0 + w * (y1 - y0)
        out = torch.where(point <= xp[0], fp[0], out)
        return torch.where(point >= xp[-1], fp[-1], out)

    def __init__(self):
        self.initial_volume_constraints: list[_VolumeWindow] = []
        self.volume_constraints: list[_VolumeWindow] = []
        self.injection_flexibility: list[_RateSchedule] = []
        self.withdrawal_flexibility: list[_RateSchedule] = []
        self.injection_costs: list[_DatedCost] = []
        self.withdrawal_costs: list[_DatedCost] = []

    # ---- volume windows ------------------------------------------------------------------------------------------
    def add_volume_constraint(self, start_date: float, end_date: float, vmin: float, vmax: float, penalty: float = 0.0) -> None:
        self.initial_volume_constraints.append(_VolumeWindow(start_date, end_date, vmin, vmax, penalty))
        self.initial_volume_constraints.sort(key=lambda w: w.start_date)

    def _get_volume_window(self, date: float, constraints: list) -> _VolumeWindow:
        return _covering(date, constraints, "No volume constraints configured.")

    def get_initial_volume_constraint(self, date: float) -> _VolumeWindow:
        return self._get_volume_window(date, self.initial_volume_constraints)

    def get_volume_constraint(self, date: float) -> _VolumeWindow:
        return self._get_volume_window(date, self.volume_constraints or self.initial_volume_constraints)

    # ---- rate curves ---------------------------------------------------------------------------------------------
    @staticmethod
    def _add_rate_schedule(container: list, start_date: float, end_date: float, point: float, rate: float) -> None:
        for sch in container:
            if math.isclose(sch.start_date, start_date, abs_tol=DATE_TOL) and math.isclose(sch.end_date, end_date, abs_tol=DATE_TOL):
                sch.values.append(_RatePoint(point, rate))
                sch.values.sort(key=lambda p: p.point)
                return
        container.append(_RateSchedule(start_date, end_date, [_RatePoint(point, rate)]))
        container.sort(key=lambda s: s.start_date)

    @staticmethod
    def _get_rate_schedule(date: float, container: list) -> list:
        return _covering(date, container, "No flexibility slice configured.").values

    def add_injection_flexibility(self, start_date: float, end_date: float, point: float, rate: float) -> None:
        self._add_rate_schedule(self.injection_flexibility, start_date, end_date, point, rate)

    def get_injection_flexibility_slice(self, date: float) -> list:
        return self._get_rate_schedule(date, self.injection_flexibility)

    def get_injection_flexibility_rate(self, date: float, point: float) -> float:
        return self._interpolate_rate(point, self.get_injection_flexibility_slice(date))

    def add_withdrawal_flexibility(self, start_date: float, end_date: float, point: float, rate: float) -> None:
        self._add_rate_schedule(self.withdrawal_flexibility, start_date, end_date, point, rate)

    def get_withdrawal_flexibility_slice(self, date: float) -> list:
        return self._get_rate_schedule(date, self.withdrawal_flexibility)

    def get_withdrawal_flexibility_rate(self, date: float, point: float) -> float:
        return self._interpolate_rate(point, self.get_withdrawal_flexibility_slice(date))

    # ---- dated costs: piecewise constant from the left -----------------------------------------------------------
    @staticmethod
    def _add_dated_cost(container: list, date: float, cost: float) -> None:
        container.append(_DatedCost(date, cost))
        container.sort(key=lambda c: c.date)

    @staticmethod
    def _get_dated_cost(date: float, container: list) -> float:
        if not container:
            raise ValueError("No variable costs configured.")
        pos = bisect_left([c.date for c in container], date)
        if pos == len(container):
            return container[-1].cost
        if pos == 0 or math.isclose(container[pos].date, date, abs_tol=DATE_TOL):
            return container[pos].cost
        return container[pos - 1].cost

    def add_variable_injection_cost(self, date: float, cost: float) -> None:
        self._add_dated_cost(self.injection_costs, date, cost)

    def get_variable_injection_cost(self, date: float) -> float:
        return self._get_dated_cost(date, self.injection_costs)

    def add_variable_withdrawal_cost(self, date: float, cost: float) -> None:
        self._add_dated_cost(self.withdrawal_costs, date, cost)

    def get_variable_withdrawal_cost(self, date: float) -> float:
        return self._get_dated_cost(date, self.withdrawal_costs)

    # ---- window optimiser ----------------------------------------------------------------------------------------
    def _tighten_boundary_to_preserve_reachability(self, date_i: float, period: float, index: int, optimize_vmax: bool,
                                                   constraints: list) -> None:
        """move a boundary of date `index` towards the next date's until the next window is reachable from it: bisection to
        1/1000 of the starting interval"""
        if optimize_vmax:
            target = constraints[index + 1].vmax
            lo, hi = target, constraints[index].vmax                   # lo always reaches the target by withdrawing
            tol = (hi - lo) / 1000.0
            gap = float("inf")
            while gap > tol:
                mid = lo + 0.5 * (hi - lo)
                if mid - self.get_withdrawal_flexibility_rate(date_i, mid) * period <= target:
                    lo = mid
                else:
                    hi = mid
                gap = hi - lo
            constraints[index].vmax = lo
            return
        target = constraints[index + 1].vmin
        hi, lo = target, constraints[index].vmin                       # hi always reaches the target by injecting
        tol = (hi - lo) / 1000.0
        gap = float("inf")
        while gap > tol:
            mid = hi - 0.5 * (hi - lo)
            if mid + self.get_injection_flexibility_rate(date_i, mid) * period <= target:
                lo = mid
            else:
                hi = mid
            gap = hi - lo
        constraints[index].vmin = hi

    def optimize_volume_constraints(self, start_date: float, end_date: float, rollout_interval: float, initial_volume: float) -> None:
        """one window per action date (and the end date), the first pinned to the initial volume; forward sweeps narrow the
        next window to what the rates can reach, a boundary that must move BACKWARDS is bisected and the sweep restarts"""
        dates, configured, windows = [], [], []
        date = start_date
        while date <= end_date + DATE_TOL:
            nxt = min(date + rollout_interval, end_date)
            w = self.get_initial_volume_constraint(date)
            vmin, vmax = w.vmin, w.vmax
            if math.isclose(date, start_date, abs_tol=DATE_TOL):
                vmin = vmax = initial_volume
            configured.append(w)
            windows.append(_VolumeWindow(date, nxt, vmin, vmax, w.penalty))
            dates.append(date)
            if date >= end_date - DATE_TOL:
                break
            date = nxt

        restart = True
        while restart:
            restart = False
            for i in range(len(windows) - 1):
                cur, nxt = windows[i], windows[i + 1]
                t, period = cur.start_date, dates[i + 1] - dates[i]
                vmax_i, vmax_n, vmin_i, vmin_n = cur.vmax, nxt.vmax, cur.vmin, nxt.vmin
                wd_at_max = self.get_withdrawal_flexibility_rate(t, vmax_i) * period
                wd_at_min = self.get_withdrawal_flexibility_rate(t, vmin_i) * period
                inj_at_max = self.get_injection_flexibility_rate(t, vmax_i) * period
                inj_at_min = self.get_injection_flexibility_rate(t, vmin_i) * period

                if vmax_i < vmax_n:
                    if vmax_i + inj_at_max < vmax_n:
                        nxt.vmax = vmax_i + inj_at_max
                elif vmax_i - wd_at_max > vmax_n:
                    self._tighten_boundary_to_preserve_reachability(t, period, i, True, windows)
                    restart = True

                if vmin_i < vmin_n:
                    if vmin_i + inj_at_min < vmin_n:
                        self._tighten_boundary_to_preserve_reachability(t, period, i, False, windows)
                        restart = True
                elif vmin_i - wd_at_min > vmin_n:
                    nxt.vmin = vmin_i - wd_at_min

                bad_i = cur.vmin > configured[i].vmax or cur.vmax < configured[i].vmin
                bad_n = nxt.vmin > configured[i + 1].vmax or nxt.vmax < configured[i + 1].vmin
                if bad_i or bad_n:
                    raise ValueError(f"Initial volume constraints cannot be satisfied at date {dates[i] if bad_i else dates[i + 1]}.")
                if restart:
                    break
        self.volume_constraints = windows
