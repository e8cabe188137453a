"""Plain numpy / fp64 restatement of v_diffusion/resample.py (the module docstring there states the semantics): the probabilities with
a sequential running sum, the draw from given uniforms and the sequential update loop with its skip rules.  No torch, no GPU."""
import math

import numpy as np


class Ref:
    def __init__(self, T, K=10, eps=0.001):
        self.T, self.K, self.eps = int(T), int(K), float(eps)
        self.hist = np.zeros((T, K), dtype=np.float32)
        self.count = np.zeros(T, dtype=np.int32)
        self.pos = np.zeros(T, dtype=np.int32)

    def warmed_up(self):
        return bool((self.count == self.K).all())

    def probabilities(self):
        """q (T,) fp64 of a warmed-up history: m_t = sqrt(sum_k h^2 / K) with k ascending, S = m_0 + m_1 + ... in order"""
        T, K = self.T, self.K
        acc = np.zeros(T, dtype=np.float64)
        for k in range(K):
            h = self.hist[:, k].astype(np.float64)
            acc = acc + h * h
        m = np.sqrt(acc / K)
        S = 0.0
        for v in m:
            S += float(v)
        if not (S > 0.0) or not math.isfinite(S):
            return np.full(T, 1.0 / T, dtype=np.float64)
        return (1.0 - self.eps) * m / S + self.eps / T

    def cdf(self):
        """C_i = q_0 + ... + q_i, sequential"""
        q = self.probabilities()
        C = np.empty_like(q)
        s = 0.0
        for i, v in enumerate(q):
            s += float(v)
            C[i] = s
        return C

    def draw(self, u):
        """(t fp64, idx int32, w fp32) from uniforms u (fp64)"""
        u = np.asarray(u, dtype=np.float64)
        T = self.T
        if self.warmed_up():
            q, C = self.probabilities(), self.cdf()
            idx = np.array([min(T - 1, int((C <= x).sum())) for x in u], dtype=np.int32)
            w = (1.0 / (T * q[idx])).astype(np.float32)
        else:
            idx = np.minimum(T - 1, np.floor(u * T)).astype(np.int32)
            w = np.ones(len(u), dtype=np.float32)
        return (idx.astype(np.float64) + 1.0) / T, idx, w

    def update(self, idx, loss):
        for i, l in zip(np.asarray(idx).tolist(), np.asarray(loss, dtype=np.float32).tolist()):
            if not 0 <= i < self.T or not math.isfinite(l):
                continue
            self.hist[i, self.pos[i]] = l
            self.pos[i] = (self.pos[i] + 1) % self.K
            self.count[i] = min(self.count[i] + 1, self.K)
