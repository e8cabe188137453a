"""Opt-in fused optimizer tail for the reference's OWN training loop (reference train.py:158, train_utils.py:159-168,
utils.py:123-190).  The reference's ``Trainer.step`` runs ``clip_grad_norm_`` -> ``torch.optim.AdamW.step`` -> ``LambdaLR.step`` ->
``EMA.update`` -- a dozen multi-tensor passes plus three launches per parameter for the EMA -- around this package's UNet.  Two edited lines of
``train.py`` put the hot path's one-pass kernels (csrc/optim.hip: vd_sumsq, vd_adamw_ema) under that loop without touching train_utils.py:

    optimizer = v_diffusion.optim.FusedAdamW(model.parameters(), lr=lr, betas=(beta1, beta2), weight_decay=weight_decay)   # was torch.optim.AdamW(...)
    v_diffusion.optim.use_fused_ema()            # the reference Trainer's ``EMA(model, decay)`` becomes v_diffusion.optim.EMA

``FusedAdamW`` moves the parameters into the flat store the hot-path trainer uses too (``flat.FlatParams``, here in ``parameters()`` order:
``param.data`` become views) and so gives every parameter a slot in one flat gradient buffer; the UNet's autograd nodes hand autograd fresh
VIEWS of those slots (models/unet.py::_grad_targets), which ``AccumulateGrad`` keeps instead of cloning, so ``param.grad`` already lies in the
flat buffer when ``step()`` runs: one vd_adamw_ema launch updates parameters and moments (``EMA.update()`` then is one ``lerp_`` over it).  Same
arithmetic as torch.optim.AdamW (decoupled weight decay, bias corrections, eps outside the square root's bias correction as torch does);
parameters that received no gradient (a class-conditional network called with y = None) are skipped with their own step count, as torch does.
``PowerEMA`` tracks the power-function profiles of post-hoc EMA (v_diffusion/phema.py) over the same flat store, with ``EMA``'s interface.
There is no CPU path: CPU parameters raise."""
import weakref

import torch

from . import _hip
from .flat import FlatParams, owner


class FusedAdamW(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=None):
        params = list(params)
        if not params or any(isinstance(p, dict) for p in params):
            raise ValueError("FusedAdamW takes ONE flat list of parameters (the reference builds a single group: train.py:158)")
        if any((not p.is_cuda) or p.dtype != torch.float32 for p in params):
            raise RuntimeError("FusedAdamW: fp32 parameters on an MI355X only (the v_diffusion hot path has no CPU fallback)")
        _hip.lib()
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, max_grad_norm=max_grad_norm))
        self.flat = FlatParams(list(enumerate(params)))              # named by position in parameters(): the AdamW state's index
        self.p, self.g, self.m, self.v = self.flat.p, self.flat.g, self.flat.m, self.flat.v
        self._params, self._offs = params, [self.flat.offsets[i] for i in range(len(params))]
        self.gnorm_sq = torch.zeros(1, dtype=torch.float32, device=params[0].device)
        self.steps = 0                  # updates of the parameters that always receive gradients
        self.lag_range = None           # (lo, hi): the ONE contiguous range that may see no gradient (class embedding), with its own count
        self.skipped = 0                # updates that range sat out (its per-parameter step of torch.optim.AdamW = steps - skipped)

    @property
    def lag_steps(self):
        return self.steps - self.skipped

    def _gather_grads(self):
        """param.grad -> the flat gradient buffer (no copy for gradients that already lie in their slot); returns the range without gradient"""
        base, missing, stray_dst, stray_src = self.g.data_ptr(), [], [], []
        for i, (p, o) in enumerate(zip(self._params, self._offs)):
            gr = p.grad
            if gr is None:
                missing.append(i)
            elif gr.data_ptr() != base + 4 * o or not gr.is_contiguous():
                stray_dst.append(self.flat.view(self.g, i)); stray_src.append(gr)
        if stray_dst:
            torch._foreach_copy_(stray_dst, stray_src)
        return self.flat.span(missing) if missing else None

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        grp = self.param_groups[0]
        lr, (b1, b2), eps, wd = float(grp["lr"]), grp["betas"], float(grp["eps"]), float(grp["weight_decay"])
        max_norm = grp.get("max_grad_norm") or 0.0
        nograd = self._gather_grads()
        if nograd is not None:
            if self.lag_range not in (None, nograd):
                raise NotImplementedError("FusedAdamW: a second range of parameters without gradients")
            self.lag_range = nograd
        self.steps += 1
        k = self.steps
        if max_norm > 0:
            _hip.sumsq(self.g, self.gnorm_sq)
        r_lo = r_hi = r_mode = 0
        r_bc1 = r_bc2 = 1.0
        if self.lag_range is not None:
            r_lo, r_hi = self.lag_range
            if nograd is not None:
                self.skipped += 1
                r_mode = 1                                                  # torch.optim.AdamW skips parameters whose .grad is None
            else:
                kl = self.lag_steps                                         # the range's own step count: updates it took part in
                r_mode, r_bc1, r_bc2 = 2, 1 - b1 ** kl, 1 - b2 ** kl
        _hip.adamw_ema(self.p, self.g, self.m, self.v, None, self.gnorm_sq if max_norm > 0 else None, float(max_norm), lr, b1, b2, eps, wd,
                       1 - b1 ** k, 1 - b2 ** k, 1.0, r_lo, r_hi, r_mode, r_bc1, r_bc2)
        return loss

    # -- torch.optim.AdamW-format state (reference checkpoints: train_utils.py:317-331 saves optimizer.state_dict())
    def state_dict(self):
        grp = {k: v for k, v in self.param_groups[0].items() if k != "params"}
        grp["params"] = list(range(len(self.flat.names)))
        return {"state": self.flat.adamw_state(self.steps, self.lag_range, self.lag_steps), "param_groups": [grp]}

    def load_state_dict(self, sd):
        grp = dict(sd["param_groups"][0])
        grp.pop("params", None)
        self.param_groups[0].update(grp)
        self.steps, self.lag_range, lag_steps = self.flat.load_adamw_state(sd["state"])
        self.skipped = self.steps - lag_steps


class EMA:
    """The reference's ``EMA`` (utils.py:123-190: same constructor, ``update / apply / restore``, context manager, ``state_dict`` with per-name
    ``shadow``) over ONE flat shadow buffer when the parameters live in a ``FusedAdamW`` flat buffer: ``update()`` is one ``lerp_`` launch instead of
    three launches per parameter, ``apply()`` / ``restore()`` copy one buffer instead of cloning every parameter.  Parameters that are not flat
    (no FusedAdamW, or one built later: the shadow moves over at the next ``update()``) take a multi-tensor ``lerp_``."""

    def __init__(self, model, decay=0.9999):
        self._named = [(k, v) for k, v in model.named_parameters() if v.requires_grad]
        self._refs = {k: weakref.ref(v) for k, v in self._named}
        self.decay = decay
        self.num_updates = 0
        self.backup = None
        self._store = None
        self.shadow = None
        self._build()

    def _build(self):
        """(re)build the shadow in the layout the parameters have NOW: flat if one flat store owns them all, in order; per tensor otherwise"""
        ps = [v for _, v in self._named]
        own = [owner(p) for p in ps]
        st = own[0][0] if own and own[0] is not None else None
        old = self.shadow
        if st is not None and len(st.names) == len(ps) and all(o is not None and o[0] is st and o[1] == i for o, i in zip(own, st.names)):
            self._store = weakref.ref(st)
            self._shadow_flat = st.p.clone()
            self.shadow = {k: st.view(self._shadow_flat, i) for i, (k, _) in zip(st.names, self._named)}
        else:
            self._store, self._shadow_flat = None, None
            self.shadow = {k: v.detach().clone() for k, v in self._named}
        if old is not None:
            with torch.no_grad():
                for k in self.shadow:
                    self.shadow[k].copy_(old[k])

    @torch.no_grad()
    def update(self):
        if self._store is None and all(owner(p) is not None for _, p in self._named):
            self._build()                                                  # the optimizer was built after this object: move the shadow
        self.num_updates += 1
        decay = min(self.decay, (1 + self.num_updates) / (10 + self.num_updates))
        st = self._store() if self._store is not None else None
        if st is not None:
            self._shadow_flat.lerp_(st.p, 1 - decay)                      # shadow += (1 - decay) (p - shadow), utils.py:144-149
        else:
            torch._foreach_lerp_([self.shadow[k] for k, _ in self._named], [r().data for r in self._refs.values()], 1 - decay)

    @torch.no_grad()
    def apply(self):
        st = self._store() if self._store is not None else None
        if st is not None:
            self.backup = st.p.clone()
            st.p.copy_(self._shadow_flat)
        else:
            self.backup = {k: r().detach().clone() for k, r in self._refs.items()}
            for k, r in self._refs.items():
                r().data.copy_(self.shadow[k])

    @torch.no_grad()
    def restore(self):
        st = self._store() if self._store is not None else None
        if st is not None and torch.is_tensor(self.backup):
            st.p.copy_(self.backup)
        else:
            for k, r in self._refs.items():
                r().data.copy_(self.backup[k])
        self.backup = None

    def __enter__(self):
        self.apply()

    def __exit__(self, *exc):
        self.restore()

    def state_dict(self):
        return {"decay": self.decay, "shadow": self.shadow, "num_updates": self.num_updates}

    @property
    def extra_states(self):
        return {"decay", "num_updates"}

    def load_state_dict(self, state_dict, strict=True):
        mine, theirs = set(self.shadow).union(self.extra_states), set(state_dict["shadow"]).union(self.extra_states)
        bad = set.symmetric_difference(mine, theirs) if strict else set.difference(mine, theirs)
        if bad:
            raise RuntimeError("Key mismatch!\n" f"Missing key(s): {', '.join(set.difference(mine, theirs))}."
                               f"Unexpected key(s): {', '.join(set.difference(theirs, mine))}")
        with torch.no_grad():
            for k, v in state_dict["shadow"].items():
                if k in self.shadow:
                    self.shadow[k].copy_(v)
        self.decay = state_dict.get("decay", self.decay)
        self.num_updates = state_dict.get("num_updates", self.num_updates)


class PowerEMA:
    """Power-function EMA profiles (post-hoc EMA, v_diffusion/phema.py) for the reference's own loop, with the interface of ``EMA``:
    ``update / apply(sigma_rel) / restore``, context manager (the first profile), ``state_dict`` / ``load_state_dict``, and ``snapshot()``,
    whose dicts ``phema.posthoc_ema`` rebuilds any profile from.  There is NO new kernel here: over a ``FusedAdamW`` store ``update()`` is
    one ``lerp_`` launch per profile over its flat shadow, at the rate ``phema.power_ema_rate`` forms in double (as ``EMA.update`` is one
    ``lerp_``); parameters that are not flat take one multi-tensor ``lerp_`` per profile.  The first update's rate is exactly 1: the
    shadow becomes the parameters.  (The fused form, every profile in the optimizer's own pass, is ``HotPathTrainer(ema_sigma_rels=...)``.)"""

    def __init__(self, model, sigma_rels=(0.05, 0.10)):
        from . import phema
        self.sigma_rels = tuple(float(s) for s in sigma_rels)
        if not self.sigma_rels or len(set(self.sigma_rels)) != len(self.sigma_rels):
            raise ValueError(f"PowerEMA: at least one width, all distinct, got {sigma_rels!r}")
        self.gammas = tuple(phema.sigma_rel_to_gamma(s) for s in self.sigma_rels)
        self._named = [(k, v) for k, v in model.named_parameters() if v.requires_grad]
        self._refs = {k: weakref.ref(v) for k, v in self._named}
        self.num_updates = 0
        self.backup = None
        self._store = None
        self.shadows = None
        self._build()

    def _build(self):
        """(re)build the shadows in the layout the parameters have NOW, as ``EMA._build`` does"""
        ps = [v for _, v in self._named]
        own = [owner(p) for p in ps]
        st = own[0][0] if own and own[0] is not None else None
        old = self.shadows
        if st is not None and len(st.names) == len(ps) and all(o is not None and o[0] is st and o[1] == i for o, i in zip(own, st.names)):
            self._store = weakref.ref(st)
            self._flat = [st.p.clone() for _ in self.sigma_rels]
            self.shadows = [{k: st.view(f, i) for i, (k, _) in zip(st.names, self._named)} for f in self._flat]
        else:
            self._store, self._flat = None, None
            self.shadows = [{k: v.detach().clone() for k, v in self._named} for _ in self.sigma_rels]
        if old is not None:
            with torch.no_grad():
                for new, was in zip(self.shadows, old):
                    for k in new:
                        new[k].copy_(was[k])

    def _index(self, sigma_rel):
        if sigma_rel is None:
            return 0
        if float(sigma_rel) not in self.sigma_rels:
            raise KeyError(f"sigma_rel {sigma_rel!r} is not tracked (tracked: {self.sigma_rels})")
        return self.sigma_rels.index(float(sigma_rel))

    @torch.no_grad()
    def update(self):
        from . import phema
        if self._store is None and all(owner(p) is not None for _, p in self._named):
            self._build()
        self.num_updates += 1
        st = self._store() if self._store is not None else None
        for j, g in enumerate(self.gammas):
            rate = phema.power_ema_rate(self.num_updates, g)
            if st is not None:
                self._flat[j].lerp_(st.p, rate)
            else:
                torch._foreach_lerp_([self.shadows[j][k] for k, _ in self._named], [r().data for r in self._refs.values()], rate)

    @torch.no_grad()
    def apply(self, sigma_rel=None):
        j = self._index(sigma_rel)
        st = self._store() if self._store is not None else None
        if st is not None:
            self.backup = st.p.clone()
            st.p.copy_(self._flat[j])
        else:
            self.backup = {k: r().detach().clone() for k, r in self._refs.items()}
            for k, r in self._refs.items():
                r().data.copy_(self.shadows[j][k])

    @torch.no_grad()
    def restore(self):
        if self.backup is None:
            raise RuntimeError("PowerEMA.restore() without a preceding apply()")
        st = self._store() if self._store is not None else None
        if st is not None and torch.is_tensor(self.backup):
            st.p.copy_(self.backup)
        else:
            for k, r in self._refs.items():
                r().data.copy_(self.backup[k])
        self.backup = None

    def __enter__(self):
        self.apply()

    def __exit__(self, *exc):
        self.restore()

    def snapshot(self):
        """the profiles as a post-hoc EMA snapshot dict (phema.py): the flat shadows as they are over a flat store, else the shadows packed
        in ``named_parameters()`` order at 4-float granules"""
        from . import phema
        st = self._store() if self._store is not None else None
        if st is not None:
            layout = [(k, st.offsets[i], tuple(p.shape)) for i, (k, p) in zip(st.names, self._named)]
            return phema.make_snapshot(self.num_updates, self.sigma_rels, layout, st.numel, self._flat)
        layout, n = [], 0
        for k, p in self._named:
            layout.append((k, n, tuple(p.shape)))
            n += (p.numel() + 3) // 4 * 4
        flats = []
        for sh in self.shadows:
            f = torch.zeros(n, dtype=torch.float32, device=self._named[0][1].device)
            for k, o, shape in layout:
                f[o:o + sh[k].numel()].copy_(sh[k].reshape(-1))
            flats.append(f)
        return phema.make_snapshot(self.num_updates, self.sigma_rels, layout, n, flats)

    def state_dict(self):
        return {"sigma_rels": list(self.sigma_rels), "shadows": self.shadows, "num_updates": self.num_updates}

    def load_state_dict(self, state_dict):
        if tuple(float(s) for s in state_dict["sigma_rels"]) != self.sigma_rels:
            raise RuntimeError(f"PowerEMA: state tracks sigma_rels {tuple(state_dict['sigma_rels'])}, this object {self.sigma_rels}")
        with torch.no_grad():
            for mine, theirs in zip(self.shadows, state_dict["shadows"]):
                if set(mine) != set(theirs):
                    raise RuntimeError(f"PowerEMA: key mismatch: {sorted(set(mine) ^ set(theirs))[:4]} ...")
                for k in mine:
                    mine[k].copy_(theirs[k])
        self.num_updates = int(state_dict["num_updates"])


def use_fused_ema():
    """Make the reference's ``Trainer`` (train_utils.py:130-133, resolved through VDIFF_REFERENCE_ROOT) build this module's ``EMA`` instead of its own:
    the one name is replaced in the LOADED reference modules; no reference file is touched."""
    import sys
    from . import _reference
    ref = _reference()
    for name in ("v_diffusion_ref.train_utils", "v_diffusion_ref.utils"):
        mod = sys.modules.get(name)
        if mod is not None and hasattr(mod, "EMA"):
            mod.EMA = EMA
    return ref
