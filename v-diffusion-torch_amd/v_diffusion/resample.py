"""Loss-aware timestep resampling, resident on the device (Nichol & Dhariwal 2021, "Improved Denoising Diffusion Probabilistic
Models", section 3.3; not part of the reference).

Trained on uniformly drawn timesteps the variational bound is too noisy a loss; drawn with p_t ~ sqrt(E[L_t^2]) and reweighted by
1/(T p_t) -- an unbiased estimate of the same sum -- it gives the paper's best likelihoods.  improved-diffusion's
``LossSecondMomentResampler`` keeps the last ten losses of every timestep in numpy, gathers every step's losses on the host and draws
with ``np.random.choice``: one device-to-host round trip per step.  ``HotPathTrainer.step`` makes none, so here the history is a
(T, K) table on the GPU and the step costs two small launches:

    vd_lsm_draw     warm-up test, root mean squares, their sum, the cumulative distribution and the B searches, one workgroup
    vd_lsm_update   the step's (timestep, loss) rows into the per-timestep rings, in row order

Semantics, with T = num_timesteps, K = history_per_term, e = uniform_prob, everything in fp64 unless stated:
    warmed up      every timestep holds K losses (decided by both kernels on the device; no host branch depends on it)
    probabilities  m_t = sqrt(sum_k hist[t, k]^2 / K), S = sum_t m_t, q_t = (1 - e) m_t / S + e / T; q_t = 1/T when S is 0 or not finite
    draw from u    warmed up: idx = min(T - 1, #{i : C_i <= u}) with C the running sum of q, w = fp32(1 / (T q_idx));
                   before that: idx = min(T - 1, floor(u T)), w = 1 exactly;  t = (idx + 1) / T either way
    update         rows in row order; a row whose index is outside [0, T) or whose loss is not finite is skipped (one NaN loss must
                   not poison a timestep for its next K visits); else hist[idx, pos[idx]] = loss, pos = (pos + 1) mod K,
                   count = min(count + 1, K)

The history of a timestep is a ring: a new loss overwrites the oldest.  improved-diffusion shifts the row and appends instead; the two
hold the same K losses in a different slot order, and only their mean of squares is ever taken.  (Its warm-up writes slot ``count``;
so does a ring that starts at slot 0.)

Random stream: ``draw(B, generator)`` consumes ONE ``torch.rand((B,), dtype=float64)`` from the generator, nothing else."""
import torch

from . import _hip

MAX_TIMESTEPS = 65536


class LossSecondMomentResampler:
    """``draw`` / ``update`` launch one kernel each and never copy state to the host.  Buffers: ``hist`` (T, K) fp32, ``count`` (T,)
    int32 (entries held, saturating at K), ``pos`` (T,) int32 (next ring slot), ``cdf`` (T,) fp64 (the distribution the last ``draw``
    used; (i + 1) / T before the history is warmed up)."""

    def __init__(self, num_timesteps, history_per_term=10, uniform_prob=0.001, device=None):
        T, K, e = int(num_timesteps), int(history_per_term), float(uniform_prob)
        if not 1 <= T <= MAX_TIMESTEPS:
            raise ValueError(f"LossSecondMomentResampler: num_timesteps must be in [1, {MAX_TIMESTEPS}], got {num_timesteps}")
        if K < 1:
            raise ValueError(f"LossSecondMomentResampler: history_per_term must be >= 1, got {history_per_term}")
        if not 0.0 <= e <= 1.0:
            raise ValueError(f"LossSecondMomentResampler: uniform_prob must be in [0, 1], got {uniform_prob}")
        device = torch.device("cuda" if device is None else device)
        if device.type != "cuda":
            raise RuntimeError("LossSecondMomentResampler: the history must live on an MI355X (there is no CPU path)")
        self.num_timesteps, self.history_per_term, self.uniform_prob, self.device = T, K, e, device
        self.hist = torch.zeros((T, K), dtype=torch.float32, device=device)
        self.count = torch.zeros((T,), dtype=torch.int32, device=device)
        self.pos = torch.zeros((T,), dtype=torch.int32, device=device)
        self.cdf = torch.zeros((T,), dtype=torch.float64, device=device)

    # ------------------------------------------------------------------ the step loop
    def draw(self, B, generator=None, u=None):
        """(t fp64 (B,), idx int32 (B,), w fp32 (B,)): B timesteps, their grid indices and the weights 1 / (T q_idx) of their losses.
        ``u`` (B fp64 uniforms in [0, 1), on the device) defaults to one ``torch.rand`` of B doubles from ``generator``."""
        B = int(B)
        if u is None:
            u = torch.rand((B,), dtype=torch.float64, device=self.device, generator=generator)
        elif u.dtype != torch.float64 or u.shape != (B,) or not u.is_contiguous():
            raise ValueError(f"LossSecondMomentResampler.draw: u must be {B} contiguous float64 values, got {u.dtype} {tuple(u.shape)}")
        t = torch.empty((B,), dtype=torch.float64, device=self.device)
        idx = torch.empty((B,), dtype=torch.int32, device=self.device)
        w = torch.empty((B,), dtype=torch.float32, device=self.device)
        _hip.lsm_draw(self.hist, self.count, u, self.cdf, t, idx, w, self.num_timesteps, self.history_per_term, B, self.uniform_prob)
        return t, idx, w

    def update(self, idx, losses):
        """``idx`` (n,) integer grid indices, ``losses`` (n,) the per-sample losses drawn at them: enter the history in row order"""
        idx, losses = idx.reshape(-1), losses.detach().reshape(-1)
        if idx.numel() != losses.numel():
            raise ValueError(f"LossSecondMomentResampler.update: {idx.numel()} indices for {losses.numel()} losses")
        idx = idx.to(torch.int32).contiguous()
        losses = losses.to(torch.float32).contiguous()
        _hip.lsm_update(self.hist, self.count, self.pos, idx, losses, idx.numel(), self.num_timesteps, self.history_per_term)

    # ------------------------------------------------------------------ inspection, checkpoints (not for the step loop)
    def probabilities(self):
        """q as (T,) fp64 on the device, by ATen from the history (1/T before the history is warmed up); no host sync"""
        T, K, e = self.num_timesteps, self.history_per_term, self.uniform_prob
        m = (self.hist.double().square().sum(1) / K).sqrt()
        S = m.sum()
        flat = torch.full_like(m, 1.0 / T)
        q = (1.0 - e) * m / S + e / T
        ok = (self.count == K).all() & (S > 0) & torch.isfinite(S)
        return torch.where(ok, q, flat)

    @property
    def warmed_up(self):
        """every timestep holds K losses; reading it synchronises: not for the step loop"""
        return bool((self.count == self.history_per_term).all().item())

    def state_dict(self):
        return {"hist": self.hist.clone(), "count": self.count.clone(), "pos": self.pos.clone(),
                "history_per_term": self.history_per_term, "uniform_prob": self.uniform_prob}

    def load_state_dict(self, sd):
        T, K = self.num_timesteps, self.history_per_term
        if int(sd["history_per_term"]) != K or tuple(sd["hist"].shape) != (T, K):
            raise RuntimeError(f"LossSecondMomentResampler: checkpoint holds a {tuple(sd['hist'].shape)} history with history_per_term = "
                               f"{sd['history_per_term']}, this object is ({T}, {K})")
        if tuple(sd["count"].shape) != (T,) or tuple(sd["pos"].shape) != (T,):
            raise RuntimeError("LossSecondMomentResampler: count / pos of the checkpoint do not have num_timesteps entries")
        e = float(sd["uniform_prob"])
        if not 0.0 <= e <= 1.0:
            raise ValueError(f"LossSecondMomentResampler: uniform_prob must be in [0, 1], got {e}")
        self.hist.copy_(sd["hist"])
        self.count.copy_(sd["count"].to(torch.int32).clamp(0, K))
        self.pos.copy_(sd["pos"].to(torch.int32).remainder(K))
        self.uniform_prob = e
