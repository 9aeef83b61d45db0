"""Allocation mechanisms: the plugin surface of src/AuctionAllocation.py:3-34.

`allocate(bids, num_slots)` keeps the reference signature and return types for one
auction; `allocate_batch(bids)` is the native form: bids [P][B] in HBM -> winners,
prices, second prices for B auctions in one kernel (ag_allocate), and
`allocate_batch(bids, num_slots)` the same for several slots (ag_allocate_slots). All run on
the GPU. Ties go to the lowest participant slot (SURVEY §8 a13'): a stable descending order;
the reference's np.argsort order among exactly tied bids is not pinned beyond that.
"""
import numpy as np
import torch

from . import _lib


class AllocationMechanism:
    """Base class for allocation mechanisms (src/AuctionAllocation.py:3-9)."""

    code = None
    _engines = {}

    def __init__(self):
        pass

    def _engine(self, P):
        from .engine import AuctionEngine
        key = (type(self), P)
        eng = AllocationMechanism._engines.get(key)
        if eng is None:
            eng = AuctionEngine(P, P, 1, 1, 0, self.code)
            AllocationMechanism._engines[key] = eng
        return eng

    def allocate_batch(self, bids, num_slots=None):
        """bids: float64 [P][B] device tensor.
        num_slots None -> one slot: (winner int32 [B], price [B], second [B]); P == 1: nobody
        is charged (SecondPrice price and every second price are NaN).
        num_slots an int, or an int32 [B] tensor of per-auction slot counts -> (winner int32
        [S][B], price [S][B], second [S][B]) with S the largest count: the arrays the reference's
        allocate returns for each auction, padded with -1 (winners) and NaN (prices)."""
        eng = self._engine(int(bids.shape[0]))
        if num_slots is None:
            return eng.allocate(bids)
        if torch.is_tensor(num_slots):
            ns = num_slots.to(device=bids.device, dtype=torch.int32)
            S = int(ns.max().item()) if ns.numel() else 1
        else:
            ns, S = None, int(num_slots)
        if not 1 <= S <= _lib.MAX_SLOTS:
            raise NotImplementedError(f"num_slots must be in 1..{_lib.MAX_SLOTS}")
        return eng.allocate_slots(bids, ns, max_slots=S)

    def allocate(self, bids, num_slots):
        """One auction, reference return types: (winners int64[min(S, P)], prices, second
        prices), the ragged arrays of src/AuctionAllocation.py:18-35."""
        num_slots = int(num_slots)
        if num_slots < 1:
            raise ValueError("num_slots must be >= 1")
        b = np.array(bids, np.float64).reshape(-1, 1)  # a copy: the caller's array may be read-only
        P = b.shape[0]
        dev = torch.from_numpy(np.ascontiguousarray(b)).cuda()
        if num_slots == 1:  # the one-slot kernel (ag_allocate)
            w, p, s = self.allocate_batch(dev)
            w, p, s = int(w.item()), float(p.item()), float(s.item())
            winners = np.array([w], dtype=np.int64)
            prices = np.array([] if np.isnan(p) else [p])
            second = np.array([] if (P < 2 or np.isnan(s)) else [s])
            return winners, prices, second
        # beyond P slots allocate returns what it returns for P slots
        n = min(num_slots, P)
        if n > _lib.MAX_SLOTS:
            raise NotImplementedError(f"more than {_lib.MAX_SLOTS} slots to fill")
        w, p, s = (t[:, 0].cpu().numpy() for t in self.allocate_batch(dev, n))
        ns = min(num_slots, P - 1)  # sorted_bids[1:num_slots + 1]
        winners = w[:n].astype(np.int64)
        prices = p[:n] if self.code == _lib.FIRST_PRICE else p[:ns]
        return winners, prices.copy(), s[:ns].copy()


class FirstPrice(AllocationMechanism):
    """(Generalised) First-Price Allocation (src/AuctionAllocation.py:11-23)."""
    code = _lib.FIRST_PRICE


class SecondPrice(AllocationMechanism):
    """(Generalised) Second-Price Allocation (src/AuctionAllocation.py:26-34)."""
    code = _lib.SECOND_PRICE
