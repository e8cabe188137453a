"""The one flat fp32 store of parameters / gradients / Adam moments, behind both ``trainer.FlatState`` (completion order) and
``optim.FusedAdamW`` (``parameters()`` order): 16-byte aligned offsets, ``param.data`` as views of ``p`` (the module, ``state_dict()``, DDP
and EMA see the same tensors as before), the one range that may see no gradient (the class embedding of a class-conditional UNet called
with y = None), and the torch.optim.AdamW-format state.  Which store owns a parameter is kept here, not on the Parameter (which stays
picklable)."""
import weakref

import torch
from torch.utils.weak import WeakIdKeyDictionary

_OWNERS = WeakIdKeyDictionary()     # Parameter -> (weak reference to its store, name); keyed by identity (a tensor's == is elementwise)


def owner(p):
    """(store, name) of a parameter that lives in a store still alive, else None"""
    e = _OWNERS.get(p)
    st = e[0]() if e is not None else None
    return None if st is None else (st, e[1])


def _padded(q):
    return (q.numel() + 3) // 4 * 4


class FlatParams:
    """``named``: (name, parameter) pairs in layout order; ``extra_grad`` floats follow the gradients in ``g_all`` (``g`` is the
    gradient part); ``state_order``: the names in ``parameters()`` order, which index the AdamW-format state (default: the layout)."""

    def __init__(self, named, extra_grad=0, state_order=None):
        self.names, self.params = [k for k, _ in named], dict(named)
        self.state_order = list(state_order or self.names)
        self.offsets, n = {}, 0
        for k, q in named:
            self.offsets[k] = n
            n += _padded(q)
        self.numel = n
        self.p, self.g_all, self.m, self.v = (torch.zeros(s, dtype=torch.float32, device=named[0][1].device) for s in (n, n + extra_grad, n, n))
        self.g = self.g_all[:n]
        self._handed = {}               # name -> weak reference to the last gradient slot view handed out (grad_slot)
        with torch.no_grad():
            for k, q in named:
                self.view(self.p, k).copy_(q)
                _OWNERS[q] = (weakref.ref(self), k)
        self.point(self.p)              # the module now lives in the flat buffer

    def view(self, buf, k):
        """parameter ``k``'s part of a flat buffer, shaped like the parameter"""
        o, q = self.offsets[k], self.params[k]
        return buf[o:o + q.numel()].view_as(q)

    def point(self, buf):
        """make every parameter's ``.data`` its part of ``buf``"""
        for k, q in self.params.items():
            q.data = self.view(buf, k)

    def span(self, names):
        """the flat range (lo, hi) of the parameters ``names``, which must be adjacent in the layout"""
        names = set(names)
        lo = min(self.offsets[k] for k in names)
        hi = max(self.offsets[k] + _padded(self.params[k]) for k in names)
        if any(lo <= o < hi for k, o in self.offsets.items() if k not in names):
            raise NotImplementedError("parameters without a gradient must be adjacent in the flat layout (the class-embedding tensors of the "
                                      "UNet are); freeze other parameters with requires_grad_(False) before building the optimizer")
        return lo, hi

    def grad_slot(self, k):
        """what a backward pass writes parameter ``k``'s gradient into: a new view of its slot in ``g`` while ``.grad`` is None and no view
        handed out earlier is alive (a gradient autograd has not delivered yet, or one ``torch.autograd.grad`` returned); else a fresh
        tensor, which the owner copies into the slot"""
        q, last = self.params[k], self._handed.get(k)
        if q.grad is not None or (last is not None and last() is not None):
            return torch.empty_like(q)
        v = self.view(self.g, k)
        self._handed[k] = weakref.ref(v)
        return v

    def adamw_state(self, steps, lag=None, lag_steps=0):
        """torch.optim.AdamW's ``state``: every parameter at ``steps``, those in the flat range ``lag`` at ``lag_steps``; a parameter at
        step 0 has no entry, as in torch"""
        state = {}
        for j, k in enumerate(self.state_order):
            s = lag_steps if lag is not None and lag[0] <= self.offsets[k] < lag[1] else steps
            if s > 0:
                state[j] = {"step": torch.tensor(float(s)), "exp_avg": self.view(self.m, k).clone(), "exp_avg_sq": self.view(self.v, k).clone()}
        return state

    @torch.no_grad()
    def load_adamw_state(self, state):
        """the moments of an AdamW ``state`` into ``m`` / ``v`` (zeros without an entry: step 0); returns (steps, lag, lag_steps) as
        ``adamw_state`` takes them"""
        self.m.zero_()
        self.v.zero_()
        steps = {}
        for j, k in enumerate(self.state_order):
            e = state.get(j, state.get(str(j)))
            steps[k] = 0 if e is None else int(float(e["step"]))
            if e is not None:
                self.view(self.m, k).copy_(e["exp_avg"])
                self.view(self.v, k).copy_(e["exp_avg_sq"])
        top, low = max(steps.values()), min(steps.values())
        if len(set(steps.values())) > 2:
            raise NotImplementedError("optimizer state: more than one group of lagging step counts")
        return top, (self.span(k for k, s in steps.items() if s == low) if low < top else None), low
