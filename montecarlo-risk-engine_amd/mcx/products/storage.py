"""Gas storage (reference surface: products/storage.py): an inventory between dated volume windows, injected into, held or
withdrawn from once per rollout interval at the spot price plus / minus a variable cost.

The product state is a REAL number in [0, S-1]: the position of the inventory inside the volume window of the date, on a grid
of S points.  The policy is Longstaff-Schwartz over that grid: per action date the regression polynomial of every grid state is
evaluated at the spot and interpolated linearly at the state each action leads to.

Host side (this file): timeline, requests, the state <-> volume maps and the three transitions on tensors (the reference's
public methods), and the per-date tables the device consumes (`_device_dates`, `_transition_table`).  The per-path work — the
backward induction over the grid and the walk of the realised state through the main simulation — is csrc/k6_storage.hip
behind mcx_storage_* (include/mcx.h); the product contributes no events to the book program."""
from __future__ import annotations

from enum import Enum

import numpy as np
import torch

from .. import _abi
from ..common.packages import FLOAT, device
from ..request_interface.request_types import AtomicRequest, AtomicRequestType
from .product import Product
from .storage_helpers import DATE_TOL, StorageConfig


class StorageAction(Enum):
    INJECTION = 0
    WITHDRAWAL = 1
    DO_NOTHING = 2


# the order in which the policy compares the actions (the first maximum wins): columns of the transition table
ACTION_ORDER = (StorageAction.INJECTION, StorageAction.DO_NOTHING, StorageAction.WITHDRAWAL)


class Storage(Product):
    is_storage = True

    def __init__(self, asset_id: str, start_date: float, end_date: float, initial_amount: float, storage_config: StorageConfig,
                 num_states: int, rollout_interval: float = 1.0):
        super().__init__(asset_ids=[asset_id])
        if num_states < 2:
            raise ValueError("Storage requires at least two discrete states.")
        if rollout_interval <= 0.0:
            raise ValueError("Rollout interval must be positive.")
        self.start_date = float(start_date)
        self.end_date = float(end_date)
        self.initial_amount = float(initial_amount)
        self.storage_config = storage_config
        self.num_states = num_states
        self.rollout_interval = float(rollout_interval)
        storage_config.optimize_volume_constraints(start_date=self.start_date, end_date=self.end_date,
                                                   rollout_interval=self.rollout_interval, initial_volume=self.initial_amount)
        actions, nexts = [], []
        t = self.start_date
        while t < self.end_date - DATE_TOL:
            nxt = min(t + self.rollout_interval, self.end_date)       # (the last period may be shorter)
            actions.append(t)
            nexts.append(nxt)
            t = nxt
        self.product_timeline = torch.tensor(actions, dtype=FLOAT, device=device)
        self.modeling_timeline = self.product_timeline
        self.regression_timeline = self.product_timeline
        self.next_action_dates = torch.tensor(nexts, dtype=FLOAT, device=device)
        self.numeraire_requests = {i: AtomicRequest(AtomicRequestType.NUMERAIRE, t) for i, t in enumerate(actions)}
        self.spot_requests = {(i, asset_id): AtomicRequest(AtomicRequestType.SPOT) for i in range(len(actions))}

    # ---- reference API -------------------------------------------------------------------------------------------
    def get_num_states(self):
        return self.num_states

    def get_state_dtype(self):
        return FLOAT

    def get_initial_state(self):
        return 0.0

    @staticmethod
    def _as_state_tensor(state) -> torch.Tensor:
        return state.to(dtype=FLOAT) if torch.is_tensor(state) else torch.tensor(state, dtype=FLOAT, device=device)

    def _window(self, date: float):
        """the (optimised) window of a date.  The config scans its windows linearly — one per action date — and every transition
        asks three times: remembered per date for as long as the config holds the same list of windows"""
        cfg = self.storage_config
        windows = cfg.volume_constraints or cfg.initial_volume_constraints
        memo = self.__dict__.get("_window_memo")
        if memo is None or memo[0] is not windows or memo[1] != len(windows):
            memo = self._window_memo = (windows, len(windows), {})
        date = float(date)
        hit = memo[2].get(date)
        if hit is None:
            hit = memo[2][date] = cfg.get_volume_constraint(date)
        return hit

    def state_to_volume(self, date: float, state) -> torch.Tensor:
        w = self._window(date)
        return w.vmin + self._as_state_tensor(state) * StorageConfig.grid_step(w.vmin, w.vmax, self.num_states)

    def _volume_to_state(self, date: float, volume: torch.Tensor) -> torch.Tensor:
        w = self._window(date)
        scale = StorageConfig.state_scale(w.vmin, w.vmax, self.num_states)
        return torch.zeros_like(volume) if scale == 0.0 else (volume - w.vmin) * scale

    def _transition_volume(self, date: float, next_date: float, action_type: StorageAction, previous_state):
        """(volume before, volume after) of one action over [date, next_date] for a tensor of states"""
        cfg, nw = self.storage_config, self._window(next_date)
        v = self.state_to_volume(date, previous_state)
        period = max(next_date - date, 0.0)
        if action_type == StorageAction.INJECTION:
            rate = cfg.interpolate_rate_tensor(v, cfg.get_injection_flexibility_slice(date))
            return v, torch.clamp(v + rate * period, max=nw.vmax)
        if action_type == StorageAction.WITHDRAWAL:
            rate = cfg.interpolate_rate_tensor(v, cfg.get_withdrawal_flexibility_slice(date))
            return v, torch.clamp(v - rate * period, min=nw.vmin)
        return v, torch.clamp(v, min=nw.vmin, max=nw.vmax)

    def compute_next_state(self, date: float, next_date: float, action_type: StorageAction):
        def mapping(previous_state) -> torch.Tensor:
            return self._volume_to_state(next_date, self._transition_volume(date, next_date, action_type, previous_state)[1])
        return mapping

    def compute_volume_difference(self, date: float, next_date: float, action_type: StorageAction):
        def mapping(previous_state) -> torch.Tensor:
            before, after = self._transition_volume(date, next_date, action_type, previous_state)
            return after - before
        return mapping

    def lookup_state_values(self, values_by_state: torch.Tensor, state_matrix: torch.Tensor) -> torch.Tensor:
        """linear interpolation of per-grid-state values [paths][S] at real-valued states [paths][B]"""
        s = torch.clamp(state_matrix.to(dtype=FLOAT), 0.0, self.num_states - 1.0)
        lo, hi = torch.floor(s).long(), torch.ceil(s).long()
        v_lo, v_hi = values_by_state.gather(1, lo), values_by_state.gather(1, hi)
        return v_lo + (s - lo.to(dtype=FLOAT)) * (v_hi - v_lo)

    # ---- native hooks --------------------------------------------------------------------------------------------
    def _cash_events(self, ctx) -> list:
        return []                 # no events in the book program: mcx_storage_eval adds this product's cashflows and exposures

    def _transition_table(self) -> np.ndarray:
        """[dates][S][3][2]: (next state, volume change) of the INTEGER grid states under [inject, hold, withdraw].  In the
        backward roll every path starts from these states, so the table is path-independent; only the spot varies."""
        states = torch.arange(self.num_states, dtype=FLOAT, device=device)
        out = np.zeros((len(self.product_timeline), self.num_states, 3, 2))
        for j, (t, nxt) in enumerate(zip(self.product_timeline.tolist(), self.next_action_dates.tolist())):
            for a, action in enumerate(ACTION_ORDER):
                before, after = self._transition_volume(t, nxt, action, states)      # (what compute_next_state / _volume_difference do)
                out[j, :, a, 0] = self._volume_to_state(nxt, after).numpy()
                out[j, :, a, 1] = (after - before).numpy()
        return out

    def _device_dates(self) -> np.ndarray:
        """one mcx_storage_date per action date (atoms and coefficient offsets are filled in by the controller)"""
        cfg, S = self.storage_config, self.num_states
        out = np.zeros(len(self.product_timeline), dtype=_abi.STORAGE_DATE_DTYPE)
        for j, (t, nxt) in enumerate(zip(self.product_timeline.tolist(), self.next_action_dates.tolist())):
            w, nw, d = self._window(t), self._window(nxt), out[j]
            d["vmin"], d["step"] = w.vmin, StorageConfig.grid_step(w.vmin, w.vmax, S)
            d["next_vmin"], d["next_vmax"] = nw.vmin, nw.vmax
            d["next_scale"] = StorageConfig.state_scale(nw.vmin, nw.vmax, S)
            d["period"] = max(nxt - t, 0.0)
            d["c_inj"], d["c_wd"] = cfg.get_variable_injection_cost(t), cfg.get_variable_withdrawal_cost(t)
            d["is_last"] = int(nxt >= self.end_date - DATE_TOL)
            for name, knots in (("inj", cfg.get_injection_flexibility_slice(t)), ("wd", cfg.get_withdrawal_flexibility_slice(t))):
                if not knots:
                    raise ValueError("Flexibility slice is empty.")
                if len(knots) > _abi.STORAGE_MAX_KNOTS:
                    raise ValueError(f"a rate curve of {len(knots)} knots exceeds MCX_STORAGE_MAX_KNOTS={_abi.STORAGE_MAX_KNOTS}")
                d["n_" + name] = len(knots)
                d[name + "_x"][:len(knots)] = [k.point for k in knots]
                d[name + "_r"][:len(knots)] = [k.rate for k in knots]
        return out
