// diffusion.hip -- fused elementwise kernels of the diffusion process (HBM / latency bound):
//   q_sample                         reference v_diffusion/diffusion.py:242-245
//   train_loss (mse) forward/backward  diffusion.py:466-490,520-541 ; flat_mean functions.py:102-104
//   one reverse step (p_mean_var + CFG + noise)  diffusion.py:317-392
//   variational-bound terms (KL / discretised decoder NLL, loss_type "kl") forward/backward  diffusion.py:446-464,497-515
//   learned variances (bound terms, hybrid loss, reverse step for outputs with variance channels)  the intent of diffusion.py:320-324
// Without a counterpart in the reference: progressive distillation; consistency distillation / training and the batched
// target-network update; the DPM-Solver++(2M) reverse step, its dynamically thresholded form and the UniPC step; the RePaint
// masked reverse step and the forward jump; the noise-map extraction of DDPM inversion; spherical interpolation; the residual and
// the corrected reverse step of Diffusion Posterior Sampling, its residual under a blur operator; the null-space reverse step of DDNM.
// All images here are NCHW, the layout of the reference call surface; the UNet converts at its own boundary.
// Device side first, then the host helpers (launch, coefficient carrier, the refusals every entry shares), then the C entries.
#include "common.h"
#include "../../include/vdiff_blur.h"

namespace {

enum { OUT_V = 0, OUT_X0 = 1, OUT_EPS = 2, OUT_BOTH = 3 };
enum { RW_CONSTANT = 0, RW_SNR = 1, RW_SNR_TRUNC = 2, RW_SNR_1PLUS = 3 };

// x0_hat = a0*xt + b0x*o[c] + b0e*o[C+c] ; eps_hat = a1*xt + b1x*o[c] + b1e*o[C+c]
struct PredCoef { float a0, b0x, b0e, a1, b1x, b1e; };

__device__ __forceinline__ PredCoef pred_coef(int type, float l) {
    const float s1 = 1.f / (1.f + expf(-l)), s0 = 1.f / (1.f + expf(l));   // sigmoid(l), sigmoid(-l)
    const float sa = sqrtf(s1), ss = sqrtf(s0);
    PredCoef k = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (type == OUT_V) { k.a0 = sa; k.b0x = -ss; k.a1 = ss; k.b1x = sa; }                       // diffusion.py:232-239
    else if (type == OUT_X0) { k.b0x = 1.f; k.a1 = rsqrtf(s0); k.b1x = -expf(0.5f * l); }         // :217-219
    else if (type == OUT_EPS) { k.a0 = rsqrtf(s1); k.b0x = -expf(-0.5f * l); k.b1x = 1.f; }       // :206-208
    else {                                                                                        // :211-214
        // x0_hat = s0*o_x + s1*(xt/alpha - o_e*sigma/alpha), eps_hat = (xt - alpha*x0_hat)/sigma, in closed form: written as
        // 1/sigma - a0*alpha/sigma the xt weight of eps_hat is a difference of two numbers near 2.2e4 at logsnr = 20 (true value 4.5e-5)
        k.a0 = sa; k.b0x = s0; k.b0e = -expf(-0.5f * l) * s1;
        k.a1 = ss; k.b1x = -sa * ss; k.b1e = s1;
    }
    return k;
}

// alpha = sqrt(sigmoid(l)), sigma = sqrt(sigmoid(-l))
struct AlphaSigma { float sa, ss; };

__device__ __forceinline__ AlphaSigma alpha_sigma(float l) { return {sqrtf(1.f / (1.f + expf(-l))), sqrtf(1.f / (1.f + expf(l)))}; }

// z_t = alpha x_0 + sigma eps: two products, each rounded, then their sum (vd_consist_pair's z_t is vd_q_sample's bit for bit:
// tests/test_consistency_gpu.py holds the two together)
__device__ __forceinline__ float q_sample_value(float x0, float eps, float sa, float ss) {
#pragma clang fp contract(off)
    return x0 * sa + eps * ss;
}

__global__ void q_sample_kernel(const float* x0, const float* eps, const float* logsnr, float* xt, long long n,
                                long long CHW) {
    const long long total = n * CHW;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (long long)gridDim.x * blockDim.x) {
        const auto [sa, ss] = alpha_sigma(logsnr[idx / CHW]);
        xt[idx] = q_sample_value(x0[idx], eps[idx], sa, ss);
    }
}

template <typename T>
__device__ __forceinline__ T block_sum(T v, T* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) sh[w] = v;
    __syncthreads();
    T t = 0;
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) t += sh[i];
    __syncthreads();
    return t;
}

struct LossArgs {
    const float* x0; const float* eps; const float* xt; const float* out;     // NCHW; out has C or 2C channels
    const float* logsnr; int type, rw; int n, C; long long HW;
};

// The MSE loss.  These two kernels and the hybrid kernels (loss_sq / loss_grad below) write the same expression, each in its own
// text: which product of a0*xt + b0x*o + b0e*oe stays unfused is the compiler's choice, and it chooses differently for the two
// spellings.  Routed through loss_sq / loss_grad, both kernels moved their snr_trunc results on an MI355X, the other reweightings
// not: 9 of 78 forward and 20 of 78 backward cases, up to 1.5e-7 of a row's loss and 4.7e-4 of a row's largest gradient (FINDINGS.md).
// one workgroup per sample
__global__ __launch_bounds__(256) void loss_fwd_kernel(const LossArgs p, float* loss, float* aux) {
    __shared__ float sh[8];
    const int b = blockIdx.x;
    const float l = p.logsnr[b];
    const PredCoef k = pred_coef(p.type, l);
    const auto [sa, ss] = alpha_sigma(l);
    float e0 = 0.f, e1 = 0.f;
    const long long N = (long long)p.C * p.HW;
    const int Co = p.type == OUT_BOTH ? 2 * p.C : p.C;
    const float* ob = p.out + (long long)b * Co * p.HW;
    for (long long i = threadIdx.x; i < N; i += blockDim.x) {
        const float x0 = p.x0[(long long)b * N + i], ep = p.eps[(long long)b * N + i];
        const float o = ob[i];
        if (p.rw == RW_SNR_TRUNC) {
            const float xt = p.xt[(long long)b * N + i];
            const float oe = p.type == OUT_BOTH ? ob[N + i] : 0.f;
            const float x0h = k.a0 * xt + k.b0x * o + k.b0e * oe;
            const float eph = k.a1 * xt + k.b1x * o + k.b1e * oe;
            e0 += (x0 - x0h) * (x0 - x0h);
            e1 += (ep - eph) * (ep - eph);
        } else {
            const float tgt = p.rw == RW_CONSTANT ? x0 : (p.rw == RW_SNR ? ep : (-x0 * ss + ep * sa));
            e0 += (tgt - o) * (tgt - o);
        }
    }
    e0 = block_sum(e0, sh);
    e1 = block_sum(e1, sh);
    if (threadIdx.x == 0) {
        const float m0 = e0 / (float)N, m1 = e1 / (float)N;
        aux[2 * b] = m0; aux[2 * b + 1] = m1;
        loss[b] = p.rw == RW_SNR_TRUNC ? fmaxf(m0, m1) : m0;
    }
}

__global__ void loss_bwd_kernel(const LossArgs p, const float* aux, const float* gloss, float* dout) {
    const long long N = (long long)p.C * p.HW, total = (long long)p.n * N;
    const int Co = p.type == OUT_BOTH ? 2 * p.C : p.C;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (long long)gridDim.x * blockDim.x) {
        const long long b = idx / N, i = idx % N;
        const float l = p.logsnr[b];
        const PredCoef k = pred_coef(p.type, l);
        const auto [sa, ss] = alpha_sigma(l);
        const float g = gloss[b] * 2.f / (float)N;
        const float* ob = p.out + b * Co * p.HW;
        float* db = dout + b * Co * p.HW;
        const float x0 = p.x0[idx], ep = p.eps[idx], o = ob[i];
        if (p.rw == RW_SNR_TRUNC) {
            const int sel = aux[2 * b] >= aux[2 * b + 1] ? 0 : 1;
            const float xt = p.xt[idx];
            const float oe = p.type == OUT_BOTH ? ob[N + i] : 0.f;
            float r, bx, be;
            if (sel == 0) { r = (k.a0 * xt + k.b0x * o + k.b0e * oe) - x0; bx = k.b0x; be = k.b0e; }
            else          { r = (k.a1 * xt + k.b1x * o + k.b1e * oe) - ep; bx = k.b1x; be = k.b1e; }
            db[i] = g * r * bx;
            if (p.type == OUT_BOTH) db[N + i] = g * r * be;
        } else {
            const float tgt = p.rw == RW_CONSTANT ? x0 : (p.rw == RW_SNR ? ep : (-x0 * ss + ep * sa));
            db[i] = g * (o - tgt);
        }
    }
}


// ---- variational bound terms (diffusion.py:446-464; normal_kl / discretized_gaussian_loglik: functions.py:31-67).
// coef[b][8] = {a0, b0x, b0e, c1, c2, true_logvar, model_logvar, a0 - 1}: x0_hat = a0*xt + b0x*o (+ b0e*o_eps),
// true_mean = c1*xt + c2*x0, model_mean = c1*xt + c2*x0_hat (the posterior mean weights do not depend on the variance type)
struct BpdArgs {
    const float* x0; const float* xt; const float* out; const float* coef; int type, clip; int n, C; long long HW;
};
constexpr float BPD_PREC = 1.f / 255.f, BPD_CUT = 0.999f, BPD_TOL = 1e-12f, CDF_K = 0.7978845608028654f, CDF_C = 0.044715f;

__device__ __forceinline__ float approx_cdf(float z) { return 0.5f * (1.f + tanhf(CDF_K * (z + CDF_C * z * z * z))); }

// one workgroup per sample: kl[b], nll[b] in bits per dimension, optional x0_hat tensor and its squared error
__global__ __launch_bounds__(256) void bpd_terms_kernel(const BpdArgs p, float* kl, float* nll, float* pred, float* mse) {
    __shared__ float sh[8];
    const int b = blockIdx.x;
    const float* k = p.coef + 8 * b;
    const float a0 = k[0], b0x = k[1], b0e = k[2], c1 = k[3], c2 = k[4], tlv = k[5], mlv = k[6], a0m1 = k[7];
    const float d = tlv - mlv, em = expf(-mlv), ed = expf(d), inv = expf(-0.5f * mlv);
    const long long N = (long long)p.C * p.HW;
    const int Co = p.type == OUT_BOTH ? 2 * p.C : p.C;
    const float* ob = p.out + (long long)b * Co * p.HW;
    float s_kl = 0.f, s_nll = 0.f, s_mse = 0.f;
    for (long long i = threadIdx.x; i < N; i += blockDim.x) {
        const float x0 = p.x0[(long long)b * N + i], xt = p.xt[(long long)b * N + i];
        const float oe = p.type == OUT_BOTH ? ob[N + i] : 0.f;
        float x0h = a0 * xt + b0x * ob[i] + b0e * oe;
        // x0_hat - x0 without forming x0_hat: at high log-SNR the difference is far below one ulp-of-x0 per cent
        float dx = fmaf(b0e, oe, fmaf(b0x, ob[i], fmaf(a0m1, xt, xt - x0)));
        if (p.clip && (x0h < -1.f || x0h > 1.f)) { x0h = fminf(fmaxf(x0h, -1.f), 1.f); dx = x0h - x0; }
        const float tm = c1 * xt + c2 * x0, mm = c1 * xt + c2 * x0h;
        s_kl += 0.5f * ((-1.f - d) + (tm - mm) * (tm - mm) * em + ed);
        const float xc = x0 - x0h;
        const float cu = x0 > BPD_CUT ? 1.f : approx_cdf(inv * (xc + BPD_PREC));
        const float cl = x0 < -BPD_CUT ? 0.f : approx_cdf(inv * (xc - BPD_PREC));
        s_nll -= logf(fmaxf(cu - cl - BPD_TOL, 0.f) + BPD_TOL);
        s_mse += dx * dx;
        if (pred) pred[(long long)b * N + i] = x0h;
    }
    s_kl = block_sum(s_kl, sh);
    s_nll = block_sum(s_nll, sh);
    s_mse = block_sum(s_mse, sh);
    if (threadIdx.x == 0) {
        const float sc = 1.f / ((float)N * 0.6931471805599453f);
        kl[b] = s_kl * sc; nll[b] = s_nll * sc;
        if (mse) mse[b] = s_mse / (float)N;
    }
}

// dout = gloss[b] * d (use_kl[b] ? kl_b : nll_b) / d out    (training runs with clip_denoised = False, diffusion.py:514)
__global__ void bpd_bwd_kernel(const BpdArgs p, const float* use_kl, const float* gloss, float* dout) {
    const long long N = (long long)p.C * p.HW, total = (long long)p.n * N;
    const int Co = p.type == OUT_BOTH ? 2 * p.C : p.C;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (long long)gridDim.x * blockDim.x) {
        const long long b = idx / N, i = idx % N;
        const float* k = p.coef + 8 * b;
        const float a0 = k[0], b0x = k[1], b0e = k[2], c1 = k[3], c2 = k[4], mlv = k[6];
        const float* ob = p.out + b * Co * p.HW;
        float* db = dout + b * Co * p.HW;
        const float x0 = p.x0[idx], xt = p.xt[idx];
        float x0h = a0 * xt + b0x * ob[i] + (p.type == OUT_BOTH ? b0e * ob[N + i] : 0.f);
        bool live = true;                                     // clamp passes no gradient outside [-1, 1]
        if (p.clip) { live = x0h >= -1.f && x0h <= 1.f; x0h = fminf(fmaxf(x0h, -1.f), 1.f); }
        float gx;                                             // d term_e / d x0_hat
        if (use_kl[b] != 0.f) {
            const float tm = c1 * xt + c2 * x0, mm = c1 * xt + c2 * x0h;
            gx = -(tm - mm) * expf(-mlv) * c2;
        } else {
            const float inv = expf(-0.5f * mlv), xc = x0 - x0h;
            const float zu = inv * (xc + BPD_PREC), zl = inv * (xc - BPD_PREC);
            const float tu = tanhf(CDF_K * (zu + CDF_C * zu * zu * zu)), tl = tanhf(CDF_K * (zl + CDF_C * zl * zl * zl));
            const float cu = x0 > BPD_CUT ? 1.f : 0.5f * (1.f + tu);
            const float cl = x0 < -BPD_CUT ? 0.f : 0.5f * (1.f + tl);
            const float D = cu - cl - BPD_TOL;
            // d cdf(z) / d x0_hat = 0.5 (1 - tanh^2) K (1 + 3 C z^2) * (-inv)
            const float du = x0 > BPD_CUT ? 0.f : 0.5f * (1.f - tu * tu) * CDF_K * (1.f + 3.f * CDF_C * zu * zu) * (-inv);
            const float dl = x0 < -BPD_CUT ? 0.f : 0.5f * (1.f - tl * tl) * CDF_K * (1.f + 3.f * CDF_C * zl * zl) * (-inv);
            gx = D >= 0.f ? -(du - dl) / (D + BPD_TOL) : 0.f;
        }
        const float g = live ? gloss[b] * gx / ((float)N * 0.6931471805599453f) : 0.f;
        db[i] = g * b0x;
        if (p.type == OUT_BOTH) db[N + i] = g * b0e;
    }
}

// ---- learned variances (Nichol & Dhariwal 2021; the reference's intent at diffusion.py:320-324 with logsnr_to_posterior :155): the
// network output has C more channels nu after its Cp = C (2C for "both") prediction channels, and per element
//   frac = sigmoid(nu),  logvar = lvmin + frac*delta,  d = lvmin - logvar = -frac*delta
// with lvmin the fixed_small (= true posterior) log-variance of the step and delta = lvmax - lvmin >= 0, both host fp64, rounded once.
// frac and 1 - frac are each formed without cancellation, so d logvar / d nu = delta*frac*(1 - frac) keeps its digits where the
// sigmoid saturates.
struct LvFrac { float frac, omf; };

__device__ __forceinline__ LvFrac lv_frac(float nu) {
    const float e = expf(-fabsf(nu)), big = 1.f / (1.f + e), small = e * big;
    return nu >= 0.f ? LvFrac{big, small} : LvFrac{small, big};
}

// written once, contraction off: the reverse step's wide and scalar forms and the bound-term kernels see the same bits
__device__ __forceinline__ float lv_logvar(float lvmin, float delta, float frac) {
#pragma clang fp contract(off)
    return __builtin_fmaf(frac, delta, lvmin);
}

// coef[b][8] = {a0, b0x, b0e, c1, c2, lvmin, delta, a0 - 1}
struct LvCoef { float a0, b0x, b0e, c1, c2, lvmin, delta, a0m1; };

__device__ __forceinline__ LvCoef lv_coef(const float* k) { return {k[0], k[1], k[2], k[3], k[4], k[5], k[6], k[7]}; }

// what forward and backward share of one element: x0_hat (clipped when asked), dx = x0_hat - x0 in the well-conditioned form of
// bpd_terms_kernel, the variance, and the two CDFs of the decoder with their arguments
struct LvElem {
    float x0h, dx, frac, omf, d, em, inv, zu, zl, tu, tl, D; bool live;
};

__device__ __forceinline__ LvElem lv_elem(const LvCoef& q, int type, int clip, float x0, float xt, float o, float oe, float nu) {
    LvElem r;
    r.x0h = q.a0 * xt + q.b0x * o + (type == OUT_BOTH ? q.b0e * oe : 0.f);
    r.dx = fmaf(q.b0e, type == OUT_BOTH ? oe : 0.f, fmaf(q.b0x, o, fmaf(q.a0m1, xt, xt - x0)));
    r.live = true;                                            // the clamp passes no gradient to the mean outside [-1, 1]
    if (clip && (r.x0h < -1.f || r.x0h > 1.f)) { r.x0h = fminf(fmaxf(r.x0h, -1.f), 1.f); r.dx = r.x0h - x0; r.live = false; }
    const LvFrac f = lv_frac(nu);
    const float lv = lv_logvar(q.lvmin, q.delta, f.frac);
    r.frac = f.frac; r.omf = f.omf;
    r.d = q.lvmin - lv;
    r.em = expf(-lv);
    r.inv = expf(-0.5f * lv);
    r.zu = r.inv * (BPD_PREC - r.dx);                         // x0 - x0_hat = -dx
    r.zl = r.inv * (-BPD_PREC - r.dx);
    r.tu = tanhf(CDF_K * (r.zu + CDF_C * r.zu * r.zu * r.zu));
    r.tl = tanhf(CDF_K * (r.zl + CDF_C * r.zl * r.zl * r.zl));
    const float cu = x0 > BPD_CUT ? 1.f : 0.5f * (1.f + r.tu);
    const float cl = x0 < -BPD_CUT ? 0.f : 0.5f * (1.f + r.tl);
    r.D = cu - cl - BPD_TOL;
    return r;
}

// KL element 0.5(-1 - d + e^d + (mean difference)^2 e^-logvar), the mean difference being c2*dx; -1 - d + e^d as expm1(d) - d
__device__ __forceinline__ float lv_kl(const LvCoef& q, const LvElem& r) {
    const float dm = q.c2 * r.dx;
    return 0.5f * ((expm1f(r.d) - r.d) + dm * dm * r.em);
}

__device__ __forceinline__ float lv_nll(const LvElem& r) { return -logf(fmaxf(r.D, 0.f) + BPD_TOL); }

// d term_e / d x0_hat (gx) and d term_e / d nu (gnu) of the KL (ukl) or the decoder NLL element
__device__ __forceinline__ void lv_grads(const LvCoef& q, const LvElem& r, float x0, bool ukl, float& gx, float& gnu) {
    float gl;                                                 // d term_e / d logvar
    if (ukl) {
        const float dm = q.c2 * r.dx;
        gx = q.c2 * dm * r.em;
        gl = 0.5f * (-expm1f(r.d) - dm * dm * r.em);
    } else {
        // cdf'(z) = 0.5 (1 - tanh^2) K (1 + 3 C z^2);  d z / d x0_hat = -inv,  d z / d logvar = -z/2
        const float pu = x0 > BPD_CUT ? 0.f : 0.5f * (1.f - r.tu * r.tu) * CDF_K * (1.f + 3.f * CDF_C * r.zu * r.zu);
        const float pl = x0 < -BPD_CUT ? 0.f : 0.5f * (1.f - r.tl * r.tl) * CDF_K * (1.f + 3.f * CDF_C * r.zl * r.zl);
        const float rD = r.D >= 0.f ? 1.f / (r.D + BPD_TOL) : 0.f;
        gx = (pu - pl) * r.inv * rD;
        gl = 0.5f * (pu * r.zu - pl * r.zl) * rD;
    }
    gnu = gl * q.delta * r.frac * r.omf;
}

// vd_bpd_terms for an output of Cp + C channels.  One workgroup per sample
__global__ __launch_bounds__(256) void bpd_terms_lv_kernel(const BpdArgs p, float* kl, float* nll, float* pred, float* mse) {
    __shared__ float sh[8];
    const int b = blockIdx.x;
    const LvCoef q = lv_coef(p.coef + 8 * b);
    const long long N = (long long)p.C * p.HW, Np = p.type == OUT_BOTH ? 2 * N : N;
    const float* ob = p.out + (long long)b * (Np + N);
    float s_kl = 0.f, s_nll = 0.f, s_mse = 0.f;
    for (long long i = threadIdx.x; i < N; i += blockDim.x) {
        const float x0 = p.x0[(long long)b * N + i], xt = p.xt[(long long)b * N + i];
        const LvElem r = lv_elem(q, p.type, p.clip, x0, xt, ob[i], p.type == OUT_BOTH ? ob[N + i] : 0.f, ob[Np + i]);
        s_kl += lv_kl(q, r);
        s_nll += lv_nll(r);
        s_mse += r.dx * r.dx;
        if (pred) pred[(long long)b * N + i] = r.x0h;
    }
    s_kl = block_sum(s_kl, sh);
    s_nll = block_sum(s_nll, sh);
    s_mse = block_sum(s_mse, sh);
    if (threadIdx.x == 0) {
        const float sc = 1.f / ((float)N * 0.6931471805599453f);
        kl[b] = s_kl * sc; nll[b] = s_nll * sc;
        if (mse) mse[b] = s_mse / (float)N;
    }
}

// dout (Cp + C channels) = gloss[b] * d (use_kl[b] ? kl_b : nll_b) / d out; without mean_grad the prediction channels are zeros
__global__ void bpd_bwd_lv_kernel(const BpdArgs p, const float* use_kl, const float* gloss, int mean_grad, float* dout) {
    const long long N = (long long)p.C * p.HW, total = (long long)p.n * N, Np = p.type == OUT_BOTH ? 2 * N : N;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (long long)gridDim.x * blockDim.x) {
        const long long b = idx / N, i = idx % N;
        const LvCoef q = lv_coef(p.coef + 8 * b);
        const float* ob = p.out + b * (Np + N);
        float* db = dout + b * (Np + N);
        const float x0 = p.x0[idx];
        const LvElem r = lv_elem(q, p.type, p.clip, x0, p.xt[idx], ob[i], p.type == OUT_BOTH ? ob[N + i] : 0.f, ob[Np + i]);
        float gx, gnu;
        lv_grads(q, r, x0, use_kl[b] != 0.f, gx, gnu);
        const float sc = gloss[b] / ((float)N * 0.6931471805599453f);
        const float g = mean_grad && r.live ? sc * gx : 0.f;
        db[i] = g * q.b0x;
        if (p.type == OUT_BOTH) db[N + i] = g * q.b0e;
        db[Np + i] = sc * gnu;
    }
}

// ---- hybrid loss (Nichol & Dhariwal 2021, eq. 16): loss_b = mse_b + vlb * (use_kl[b] ? kl_b : nll_b), mse_b loss_fwd_kernel's on the
// prediction channels and the bound term bpd_terms_lv_kernel's without clipping, whose mean is a constant to the gradient.
// aux[b][4] = {the two snr_trunc means, kl_b, nll_b}.
// The mse part is loss_fwd_kernel's and loss_bwd_kernel's expression per element, as values: the squared errors one element adds
// (e1: the eps error of snr_trunc, else 0) and their gradient g * d e / d out (ge: for the second half of a "both" output).
struct SqErr { float e0, e1; };
struct OutGrad { float gx, ge; };

__device__ __forceinline__ SqErr loss_sq(int rw, const PredCoef& k, float sa, float ss, float x0, float ep, float xt, float o, float oe) {
    if (rw == RW_SNR_TRUNC) {
        const float x0h = k.a0 * xt + k.b0x * o + k.b0e * oe;
        const float eph = k.a1 * xt + k.b1x * o + k.b1e * oe;
        return {(x0 - x0h) * (x0 - x0h), (ep - eph) * (ep - eph)};
    }
    const float tgt = rw == RW_CONSTANT ? x0 : (rw == RW_SNR ? ep : (-x0 * ss + ep * sa));
    return {(tgt - o) * (tgt - o), 0.f};
}

__device__ __forceinline__ OutGrad loss_grad(int rw, const PredCoef& k, float sa, float ss, bool eps_branch, float g, float x0, float ep,
                                             float xt, float o, float oe) {
    if (rw == RW_SNR_TRUNC) {
        float r, bx, be;
        if (!eps_branch) { r = (k.a0 * xt + k.b0x * o + k.b0e * oe) - x0; bx = k.b0x; be = k.b0e; }
        else             { r = (k.a1 * xt + k.b1x * o + k.b1e * oe) - ep; bx = k.b1x; be = k.b1e; }
        return {g * r * bx, g * r * be};
    }
    const float tgt = rw == RW_CONSTANT ? x0 : (rw == RW_SNR ? ep : (-x0 * ss + ep * sa));
    return {g * (o - tgt), 0.f};
}

// one workgroup per sample
__global__ __launch_bounds__(256) void hybrid_fwd_kernel(const LossArgs p, const float* coef, const float* use_kl, float vlb, float* loss,
                                                         float* aux) {
    __shared__ float sh[8];
    const int b = blockIdx.x;
    const float l = p.logsnr[b];
    const PredCoef k = pred_coef(p.type, l);
    const auto [sa, ss] = alpha_sigma(l);
    const LvCoef q = lv_coef(coef + 8 * b);
    const long long N = (long long)p.C * p.HW, Np = p.type == OUT_BOTH ? 2 * N : N;
    const float* ob = p.out + (long long)b * (Np + N);
    float e0 = 0.f, e1 = 0.f, s_kl = 0.f, s_nll = 0.f;
    for (long long i = threadIdx.x; i < N; i += blockDim.x) {
        const long long idx = (long long)b * N + i;
        const float x0 = p.x0[idx], xt = p.xt[idx], o = ob[i], oe = p.type == OUT_BOTH ? ob[N + i] : 0.f;
        const SqErr m = loss_sq(p.rw, k, sa, ss, x0, p.eps[idx], xt, o, oe);
        e0 += m.e0; e1 += m.e1;
        const LvElem r = lv_elem(q, p.type, 0, x0, xt, o, oe, ob[Np + i]);
        s_kl += lv_kl(q, r);
        s_nll += lv_nll(r);
    }
    e0 = block_sum(e0, sh);
    e1 = block_sum(e1, sh);
    s_kl = block_sum(s_kl, sh);
    s_nll = block_sum(s_nll, sh);
    if (threadIdx.x == 0) {
        const float m0 = e0 / (float)N, m1 = e1 / (float)N, sc = 1.f / ((float)N * 0.6931471805599453f);
        const float kl = s_kl * sc, nll = s_nll * sc;
        aux[4 * b] = m0; aux[4 * b + 1] = m1; aux[4 * b + 2] = kl; aux[4 * b + 3] = nll;
        loss[b] = (p.rw == RW_SNR_TRUNC ? fmaxf(m0, m1) : m0) + vlb * (use_kl[b] != 0.f ? kl : nll);
    }
}

// the whole gradient in one pass: the prediction channels take the mse gradient alone, the nu channels vlb * gloss[b] * d term_b / d nu
__global__ void hybrid_bwd_kernel(const LossArgs p, const float* coef, const float* use_kl, float vlb, const float* aux, const float* gloss,
                                  float* dout) {
    const long long N = (long long)p.C * p.HW, total = (long long)p.n * N, Np = p.type == OUT_BOTH ? 2 * N : N;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (long long)gridDim.x * blockDim.x) {
        const long long b = idx / N, i = idx % N;
        const float l = p.logsnr[b];
        const PredCoef k = pred_coef(p.type, l);
        const auto [sa, ss] = alpha_sigma(l);
        const LvCoef q = lv_coef(coef + 8 * b);
        const float* ob = p.out + b * (Np + N);
        float* db = dout + b * (Np + N);
        const float x0 = p.x0[idx], xt = p.xt[idx], o = ob[i], oe = p.type == OUT_BOTH ? ob[N + i] : 0.f;
        const LvElem r = lv_elem(q, p.type, 0, x0, xt, o, oe, ob[Np + i]);
        float gx, gnu;
        lv_grads(q, r, x0, use_kl[b] != 0.f, gx, gnu);
        const OutGrad m = loss_grad(p.rw, k, sa, ss, !(aux[4 * b] >= aux[4 * b + 1]), gloss[b] * 2.f / (float)N, x0, p.eps[idx], xt, o, oe);
        db[i] = m.gx;
        if (p.type == OUT_BOTH) db[N + i] = m.ge;
        db[Np + i] = vlb * gloss[b] / ((float)N * 0.6931471805599453f) * gnu;
    }
}

inline int grid_for(long long total) {
    long long g = (total + 255) / 256;
    if (g > 4096) g = 4096;
    return (int)(g < 1 ? 1 : g);
}

// V = floats per lane and access: 4 (dwordx4) when C*HW is a multiple of 4 and every base is 16-byte aligned -- a vector then never
// straddles two samples or the two halves of a "both" output -- else 1.  (2, dwordx2: the two-float rows of ddnm_step_kernel.)
template <int V> __device__ __forceinline__ void ldv(const float* p, float (&r)[V]) {
    if constexpr (V == 4) { const float4 t = *reinterpret_cast<const float4*>(p); r[0] = t.x; r[1] = t.y; r[2] = t.z; r[3] = t.w; }
    else if constexpr (V == 2) { const float2 t = *reinterpret_cast<const float2*>(p); r[0] = t.x; r[1] = t.y; }
    else r[0] = *p;
}

template <int V> __device__ __forceinline__ void stv(float* p, const float (&r)[V]) {
    if constexpr (V == 4) *reinterpret_cast<float4*>(p) = make_float4(r[0], r[1], r[2], r[3]);
    else if constexpr (V == 2) *reinterpret_cast<float2*>(p) = make_float2(r[0], r[1]);
    else *p = r[0];
}

// elements [i, i + V) of row b of xn <- r, and of rows 2b, 2b+1 of xdup (optional: the next guided network input)
template <int V> __device__ __forceinline__ void st_dup(float* xn, float* xdup, long long b, long long N, long long i, const float (&r)[V]) {
    stv<V>(xn + b * N + i, r);
    if (xdup) { stv<V>(xdup + 2 * b * N + i, r); stv<V>(xdup + (2 * b + 1) * N + i, r); }
}

// ---- what the reverse-step kernels share: the product sampler's step, the DPM-Solver++ step and its thresholded form, the RePaint step
// and the noise extraction of DDPM inversion.  Each takes the state xt (n rows of N = C*HW floats) and a network output of n*(1+cfg)
// rows, cond and uncond interleaved (diffusion.py:369-372), of N floats or, for "both", 2N (the row stride may be larger); each forms a value per branch, guides it,
// and writes xn and (optional) xdup.  The coefficients come as host floats copied into the kernel argument or, to keep the launch
// HIP-graph replayable, as a device pointer.
struct Coefs { float k[16]; const float* kdev; };     // (16: the widest row, vd_unipc_step's)

__device__ __forceinline__ const float* coefs(const Coefs& c) { return c.kdev ? c.kdev : c.k; }

struct StepCommon {
    const float* xt; const float* out; Coefs c; int type, cfg, last, clip; float* xn; float* xdup; int n; long long N;
    long long row;      // floats per row of out: N, for "both" 2N, and N more when the network also gives the variance channels
};

// Every expression of these kernels is written once, with contraction off and the fused operations spelled out: the bits of a step are
// a property of this text, not of the compiler.  The wide and the scalar form of a kernel (a caller's buffers decide between them)
// agree bit for bit, the thresholded solver step with s_max = 1 and no guidance is the solver step with clip = 1, the selection passes
// of the thresholded step see the bits its final pass sees, and noise extraction forms the mean the RePaint step forms.
__device__ __forceinline__ float x0_hat(float a0, float b0x, float b0e, bool both, float z, float o, float oe) {
#pragma clang fp contract(off)
    const float e = both ? b0e * oe : 0.f;
    return __builtin_fmaf(b0x, o, a0 * z) + e;
}

__device__ __forceinline__ float guide(float w, float xc, float xu) {
#pragma clang fp contract(off)
    return __builtin_fmaf(w, xc - xu, xc);
}

__device__ __forceinline__ float solver_update(float c1, float c2, float c2r, float z, float g, float h) {
#pragma clang fp contract(off)
    return __builtin_fmaf(c2r, g - h, __builtin_fmaf(c1, z, c2 * g));
}

// UniPC: the corrector of the step that arrived, xt + eg*(g - h0) + e1*(h1 - h0) + e2*(h2 - h0), and the predictor of the step that
// leaves, c1*xc + c2*g + p1*(h0 - g) + p2*(h1 - g): left to right, each product folded into the sum before it.  With e = 0 the first
// returns xt itself; with p2 = 0 and p1 = -c2rho the second is solver_update with the sign moved from the weight into the difference.
__device__ __forceinline__ float unipc_correct(float eg, float e1, float e2, float z, float g, float h0, float h1, float h2) {
#pragma clang fp contract(off)
    return __builtin_fmaf(e2, h2 - h0, __builtin_fmaf(e1, h1 - h0, __builtin_fmaf(eg, g - h0, z)));
}

__device__ __forceinline__ float unipc_predict(float c1, float c2, float p1, float p2, float xc, float g, float h0, float h1) {
#pragma clang fp contract(off)
    return __builtin_fmaf(p2, h1 - g, __builtin_fmaf(p1, h0 - g, __builtin_fmaf(c1, xc, c2 * g)));
}

// The posterior mean c1*z + c2*x0h + c3*o has two groupings, and they differ in the last bit: mean_plain is the product sampler's
// (three products, two sums, nothing fused), mean_fused the RePaint step's and the noise extraction's.  Both stay: merging them
// changes the bits of one side's seeded chains.
__device__ __forceinline__ float mean_plain(float c1, float c2, float c3, float z, float x0h, float o) {
#pragma clang fp contract(off)
    return c3 * o + (c1 * z + c2 * x0h);
}

__device__ __forceinline__ float mean_fused(float c1, float c2, float c3, float z, float x0h, float o) {
#pragma clang fp contract(off)
    return __builtin_fmaf(c3, o, __builtin_fmaf(c2, x0h, c1 * z));
}

__device__ __forceinline__ float axpby(float a, float x, float b, float y) {
#pragma clang fp contract(off)
    return __builtin_fmaf(b, y, a * x);
}

// per branch: the x0 prediction a0*z + b0x*o (+ b0e*o_eps), clipped to [-1, 1] when asked
struct PredX0 {
    float a0, b0x, b0e; bool both, clip;
    __device__ __forceinline__ float raw(float z, float o, float oe) const { return x0_hat(a0, b0x, b0e, both, z, o, oe); }
    __device__ __forceinline__ float clipped(float x0h) const { return clip ? fminf(fmaxf(x0h, -1.f), 1.f) : x0h; }
    __device__ __forceinline__ float operator()(float z, float o, float oe) const { return clipped(raw(z, o, oe)); }
    // 1 where the clip passes the gradient on: no clip, or -1 <= x0h <= 1 (torch.clamp's subgradient, boundary included; a NaN passes none)
    __device__ __forceinline__ float pass(float x0h) const { return (!clip || (x0h >= -1.f && x0h <= 1.f)) ? 1.f : 0.f; }
};

// per branch: the step mean c1*z + c2*x0_hat + c3*o in one of its two groupings, or x0_hat itself on the last step
// (c3 = k[7]: the weight of the raw network output, for the posterior over (eps, x0) of an eps-network without clipping, where the
// reference takes the output itself as eps, diffusion.py:338-347 -- rebuilding it as (xt - alpha*x0_hat)/sigma cancels)
template <bool FUSED> struct StepMean {
    PredX0 x0; float c1, c2, c3; bool last;
    __device__ __forceinline__ float operator()(float z, float o, float oe) const { return of(z, x0(z, o, oe), o); }
    // ... from a prediction already formed (a kernel that needs the prediction too forms it once)
    __device__ __forceinline__ float of(float z, float x0h, float o) const {
        if (last) return x0h;
        return FUSED ? mean_fused(c1, c2, c3, z, x0h, o) : mean_plain(c1, c2, c3, z, x0h, o);
    }
};

// k = {a0, b0x, b0e, c1, c2, noise scale | c2*rho, w_guide, c3 [, ak, bk]}
__device__ __forceinline__ PredX0 pred_x0(const StepCommon& s, const float* k) { return {k[0], k[1], k[2], s.type == OUT_BOTH, s.clip != 0}; }

template <bool FUSED> __device__ __forceinline__ StepMean<FUSED> step_mean(const StepCommon& s, const float* k) {
    return {pred_x0(s, k), k[3], k[4], k[7], s.last != 0};
}

// g[j] = f(z[j], o, o_eps) of sample b's cond row, guided by the same of its uncond row when cfg, for the elements [i, i + V)
template <int V, class F>
__device__ __forceinline__ void guided(const StepCommon& s, long long b, long long i, float w, const float (&z)[V], const F& f,
                                       float (&g)[V]) {
    const bool both = s.type == OUT_BOTH;
    const long long N = s.N, row = s.row;
    const float* oc = s.out + b * (1 + s.cfg) * row + i;
    float o[V], oe[V] = {};
    ldv<V>(oc, o);
    if (both) ldv<V>(oc + N, oe);
#pragma unroll
    for (int j = 0; j < V; ++j) g[j] = f(z[j], o[j], oe[j]);
    if (s.cfg) {
        ldv<V>(oc + row, o);
        if (both) ldv<V>(oc + row + N, oe);
#pragma unroll
        for (int j = 0; j < V; ++j) g[j] = guide(w, g[j], f(z[j], o[j], oe[j]));
    }
}

struct StepArgs { StepCommon s; const float* noise; };

__device__ __forceinline__ float lv_sigma(float lvmin, float delta, float nu) { return expf(0.5f * lv_logvar(lvmin, delta, lv_frac(nu).frac)); }

// one reverse step for a batch sharing the step index: xn = guided mean_plain + sigma * noise.
// Fixed variance (LV = false): sigma = k[5], added whenever noise is given, on the last step too.
// Learned variances (LV = true; s.row = prediction channels + N): k = {a0, b0x, b0e, c1, c2, lvmin, w_guide, c3, delta, 0} and per
// element sigma = exp(0.5 (lvmin + delta*sigmoid(nu))), nu the variance channels of the CONDITIONAL row (diffusion.py:386-387), added
// when noise is given and the step is not the last.  Without noise the two forms agree bit for bit on the prediction channels.
template <int V, bool LV>
__global__ void sample_step_kernel(const StepArgs p) {
    const StepCommon& s = p.s;
    const long long N = s.N, total = (long long)s.n * N / V;
    const float* k = coefs(s.c);
    const StepMean<false> f = step_mean<false>(s, k);
    const float k5 = k[5], w = k[6], delta = LV ? k[8] : 0.f;             // (k5: the noise scale, or lvmin)
    const bool noisy = p.noise && !(LV && s.last);
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const long long e = idx * V, b = e / N, i = e % N;
        float z[V], v[V];
        ldv<V>(s.xt + e, z);
        guided<V>(s, b, i, w, z, f, v);
        if (noisy) {
            float nu[V] = {}, nz[V];
            if constexpr (LV) ldv<V>(s.out + b * (1 + s.cfg) * s.row + (s.row - N) + i, nu);
            ldv<V>(p.noise + e, nz);
#pragma unroll
            for (int j = 0; j < V; ++j) v[j] = axpby(1.f, v[j], LV ? lv_sigma(k5, delta, nu[j]) : k5, nz[j]);
        }
        st_dup<V>(s.xn, s.xdup, b, N, i, v);
    }
}

// ---- progressive distillation (Salimans & Ho 2022): two DDIM steps of a teacher on the 2N grid become the regression target of one
// student step on the N grid.  coef[b][20], per sample (host, fp64, rounded once; layout in include/vdiff_hip.h):
//   0..2  teacher weights at t:   x_hat  = a0*z_t  + b0x*o (+ b0e*o_eps)         3,4  z_t' = c1*z_t + c2*x_hat
//   5..7  teacher weights at t':  x_hat' = a0*z_t' + b0x*o (+ b0e*o_eps)         8,9  x_tilde = w1*x_hat + w2*x_hat'  (w1 + w2 = 1)
//   10..12 student weights at t    13 omega   14 w_guide   15 logsnr(t), not read here
//   16,17,18  a0 - 1 of the three predictions, 19  c1 + c2 - 1, each rounded on its own
// Every prediction is formed twice: directly (what the next network pass and the caller see) and as its DIFFERENCE from the state it
// was predicted from, (a0 - 1)*z + b0x*o (+ b0e*o_eps).  The residual x_student - x_tilde is assembled from the differences alone:
// at high log-SNR all predictions sit within 1e-3 ... 1e-5 of z_t, and through the direct forms one fp32 ulp of a weight near 1 is
// up to 1e-3 of the residual (the a0 - 1 slot of the bound-term kernels, for the same reason).
enum { DK = 20 };

// guided x0 prediction x of elements [i, i + V) of sample b, and d = x - z in difference form, from a network output of n*(1+cfg)
// rows (cond, uncond interleaved): the arithmetic of sample_step_kernel's last step -- clip each prediction, then x_c + w (x_c - x_u)
template <int V>
__device__ __forceinline__ void guided_x0(const float* out, long long b, long long N, long long i, int type, int cfg, int clip, float a0,
                                          float a0m1, float b0x, float b0e, float w, const float (&z)[V], float (&x)[V], float (&d)[V]) {
    const int mul = 1 + cfg, Co = type == OUT_BOTH ? 2 : 1;
    float pr[2][V], df[2][V];
    for (int u = 0; u < mul; ++u) {
        const float* ob = out + (b * mul + u) * Co * N + i;
        float o[V], oe[V];
        ldv<V>(ob, o);
        if (type == OUT_BOTH) ldv<V>(ob + N, oe);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const float e = type == OUT_BOTH ? b0e * oe[j] : 0.f;
            float x0h = a0 * z[j] + b0x * o[j] + e;
            float dx = a0m1 * z[j] + b0x * o[j] + e;
            if (clip && (x0h < -1.f || x0h > 1.f)) { x0h = fminf(fmaxf(x0h, -1.f), 1.f); dx = x0h - z[j]; }
            pr[u][j] = x0h; df[u][j] = dx;
        }
    }
#pragma unroll
    for (int j = 0; j < V; ++j) {
        x[j] = cfg ? pr[0][j] + w * (pr[0][j] - pr[1][j]) : pr[0][j];
        d[j] = cfg ? df[0][j] + w * (df[0][j] - df[1][j]) : df[0][j];
    }
}

struct DistillMidArgs {
    const float* zt; const float* out; const float* coef; int type, cfg, clip; float* xhat; float* dhat; float* zmid; float* zdup;
    int n; long long N;
};

// teacher prediction at t (x_hat, and d_hat = x_hat - z_t) and the DDIM step to t' = t - 1/(2N); zdup (optional) = z_t' on 2n interleaved
// rows, the next guided teacher input
template <int V>
__global__ void distill_mid_kernel(const DistillMidArgs p) {
    const long long N = p.N, total = (long long)p.n * N / V;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const long long e = idx * V, b = e / N, i = e % N;
        const float* k = p.coef + DK * b;
        float z[V], x[V], d[V], zm[V];
        ldv<V>(p.zt + e, z);
        guided_x0<V>(p.out, b, N, i, p.type, p.cfg, p.clip, k[0], k[16], k[1], k[2], k[14], z, x, d);
        const float c1 = k[3], c2 = k[4];
#pragma unroll
        for (int j = 0; j < V; ++j) zm[j] = c1 * z[j] + c2 * x[j];
        stv<V>(p.xhat + e, x);
        stv<V>(p.dhat + e, d);
        stv<V>(p.zmid + e, zm);
        if (p.zdup) { stv<V>(p.zdup + 2 * b * N + i, zm); stv<V>(p.zdup + (2 * b + 1) * N + i, zm); }
    }
}

struct DistillLossArgs {
    const float* xhat; const float* dhat; const float* zmid; const float* tout; const float* zt; const float* sout; const float* coef;
    int ttype, stype, cfg, clip; int n; long long N;
};

// one workgroup per sample, fixed summation order: loss[b] = omega * mean(resid^2), resid = x_student - x_tilde from the differences:
//   z_t' - z_t = (c1 + c2 - 1) z_t + c2 d_hat,  x_hat' - z_t = d_hat' + (z_t' - z_t),  x_tilde - z_t = w1 d_hat + w2 (x_hat' - z_t)
template <int V>
__global__ __launch_bounds__(256) void distill_loss_fwd_kernel(const DistillLossArgs p, float* loss, float* resid, float* xtilde) {
    __shared__ double sh[8];
    const long long b = blockIdx.x, N = p.N;
    const float* k = p.coef + DK * b;
    const float c2 = k[4], w1 = k[8], w2 = k[9], sa0m1 = k[18], sb0x = k[11], sb0e = k[12], c12m1 = k[19];
    const float* sb = p.sout + b * (p.stype == OUT_BOTH ? 2 : 1) * N;
    double acc = 0.0;                 // squares summed in fp64 (free under the loads): the loss carries the residuals' error, not the sum's
    for (long long i = (long long)threadIdx.x * V; i < N; i += (long long)blockDim.x * V) {
        float z[V], zm[V], dh[V], xp[V], dp[V], so[V], soe[V], r[V];
        ldv<V>(p.zt + b * N + i, z);
        ldv<V>(p.zmid + b * N + i, zm);
        ldv<V>(p.dhat + b * N + i, dh);
        guided_x0<V>(p.tout, b, N, i, p.ttype, p.cfg, p.clip, k[5], k[17], k[6], k[7], k[14], zm, xp, dp);
        ldv<V>(sb + i, so);
        if (p.stype == OUT_BOTH) ldv<V>(sb + N + i, soe);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const float dz = c12m1 * z[j] + c2 * dh[j];
            const float dt = w1 * dh[j] + w2 * (dp[j] + dz);
            const float ds = sa0m1 * z[j] + sb0x * so[j] + (p.stype == OUT_BOTH ? sb0e * soe[j] : 0.f);
            r[j] = ds - dt;
            acc += (double)r[j] * (double)r[j];
        }
        stv<V>(resid + b * N + i, r);
        if (xtilde) {                                  // the target itself, in the direct (convex) form
            float xh[V], xt[V];
            ldv<V>(p.xhat + b * N + i, xh);
#pragma unroll
            for (int j = 0; j < V; ++j) xt[j] = w1 * xh[j] + w2 * xp[j];
            stv<V>(xtilde + b * N + i, xt);
        }
    }
    acc = block_sum(acc, sh);
    if (threadIdx.x == 0) loss[b] = (float)((double)k[13] * (acc / (double)N));
}

// dout = gloss[b] * omega_b * 2/N * resid * b0x (second half of a "both" student: * b0e)
template <int V>
__global__ void distill_loss_bwd_kernel(const float* resid, const float* coef, const float* gloss, int stype, float* dout, int n,
                                        long long N) {
    const long long total = (long long)n * N / V;
    const int Co = stype == OUT_BOTH ? 2 : 1;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const long long e = idx * V, b = e / N, i = e % N;
        const float* k = coef + DK * b;
        const float g = gloss[b] * k[13] * 2.f / (float)N, bx = k[11], be = k[12];
        float r[V], d[V];
        ldv<V>(resid + e, r);
#pragma unroll
        for (int j = 0; j < V; ++j) d[j] = g * r[j] * bx;
        stv<V>(dout + b * Co * N + i, d);
        if (stype == OUT_BOTH) {
#pragma unroll
            for (int j = 0; j < V; ++j) d[j] = g * r[j] * be;
            stv<V>(dout + b * Co * N + N + i, d);
        }
    }
}

// ---- consistency distillation / training (Song et al. 2023; Song & Dhariwal 2024): the student at (z_t, t) regresses on a target
// network at (z_s, s = t - 1/N), z_s one DDIM step of a teacher down from z_t (distillation) or the same x_0, eps noised to s
// (training).  coef[n][24], see include/vdiff_hip.h.  As above the residual is assembled from differences: each prediction minus
// the state it was made from, and dz = z_s - z_t from weights rounded on their own -- never from two nearly equal images.
// The expressions are spelled out with contraction off: the wide and the scalar form give the same bits.
enum { CK = 24, CK_LAST = 22 };

__device__ __forceinline__ float consist_diff(float a0m1, float b0x, float b0e, bool both, float z, float o, float oe) {
#pragma clang fp contract(off)
    const float e = both ? b0e * oe : 0.f;
    return __builtin_fmaf(b0x, o, a0m1 * z) + e;
}

struct ConsistMidArgs {
    const float* zt; const float* out; const float* coef; int type, cfg, clip; float* zs; float* dz; float* xhat; int n; long long N;
};

// teacher prediction at t (guided_x0: x_hat and d_hat = x_hat - z_t) and the DDIM step to s: z_s = c1 z_t + c2 x_hat,
// dz = (c1 + c2 - 1) z_t + c2 d_hat; rows with i = 1 (s = 0) take x_hat and d_hat themselves
template <int V>
__global__ void consist_mid_kernel(const ConsistMidArgs p) {
    const long long N = p.N, total = (long long)p.n * N / V;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const long long e = idx * V, b = e / N, i = e % N;
        const float* k = p.coef + CK * b;
        float z[V], x[V], d[V], zs[V], dz[V];
        ldv<V>(p.zt + e, z);
        guided_x0<V>(p.out, b, N, i, p.type, p.cfg, p.clip, k[0], k[14], k[1], k[2], k[12], z, x, d);
        const float c1 = k[3], c2 = k[4], c12m1 = k[17];
        const bool last = k[CK_LAST] != 0.f;
#pragma unroll
        for (int j = 0; j < V; ++j) {
            zs[j] = last ? x[j] : axpby(c1, z[j], c2, x[j]);
            dz[j] = last ? d[j] : axpby(c12m1, z[j], c2, d[j]);
        }
        stv<V>(p.zs + e, zs);
        stv<V>(p.dz + e, dz);
        if (p.xhat) stv<V>(p.xhat + e, x);
    }
}

// training mode: z_t (q_sample), z_s = alpha_s x_0 + sigma_s eps and dz = (alpha_s - alpha_t) x_0 + (sigma_s - sigma_t) eps in one pass
template <int V>
__global__ void consist_pair_kernel(const float* x0, const float* eps, const float* coef, float* zt, float* zs, float* dz, int n,
                                    long long N) {
    const long long total = (long long)n * N / V;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const long long e = idx * V, b = e / N;
        const float* k = coef + CK * b;
        const float l = k[13], da = k[18], ds = k[19], as = k[20], ss = k[21];
        const auto [sat, sst] = alpha_sigma(l);
        float x[V], ep[V], a[V], s[V], d[V];
        ldv<V>(x0 + e, x);
        ldv<V>(eps + e, ep);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            a[j] = q_sample_value(x[j], ep[j], sat, sst);
            s[j] = axpby(as, x[j], ss, ep[j]);
            d[j] = axpby(da, x[j], ds, ep[j]);
        }
        stv<V>(zt + e, a);
        stv<V>(zs + e, s);
        stv<V>(dz + e, d);
    }
}

struct ConsistLossArgs {
    const float* zt; const float* zs; const float* dz; const float* sout; const float* tout; const float* coef; int type, metric;
    double c; int n; long long N;
};

// one workgroup per sample, fixed summation order.  resid = [student - z_t] - [target - z_s] - dz; rows with i = 1 SELECT the
// boundary condition (target = z_s, its bracket 0) and never read the target network's output.  S = sum resid^2 in fp64;
// metric 0 (l2): loss = omega S/N, aux = 2/N;  metric 1 (pseudo-Huber): loss = omega S/(sqrt(S + c^2) + c), aux = 1/sqrt(S + c^2)
template <int V>
__global__ __launch_bounds__(256) void consist_loss_fwd_kernel(const ConsistLossArgs p, float* loss, float* resid, float* aux,
                                                               float* target) {
    __shared__ double sh[8];
    const long long b = blockIdx.x, N = p.N;
    const float* k = p.coef + CK * b;
    const bool both = p.type == OUT_BOTH, last = k[CK_LAST] != 0.f;
    const int Co = both ? 2 : 1;
    const float ga0 = k[5], gb0x = k[6], gb0e = k[7], sb0x = k[9], sb0e = k[10], ga0m1 = k[15], sa0m1 = k[16];
    const float* sb = p.sout + b * Co * N;
    const float* tb = p.tout + b * Co * N;
    double acc = 0.0;
    for (long long i = (long long)threadIdx.x * V; i < N; i += (long long)blockDim.x * V) {
        float z[V], zs[V], dz[V], so[V], soe[V] = {}, go[V] = {}, goe[V] = {}, r[V];
        ldv<V>(p.zt + b * N + i, z);
        ldv<V>(p.zs + b * N + i, zs);
        ldv<V>(p.dz + b * N + i, dz);
        ldv<V>(sb + i, so);
        if (both) ldv<V>(sb + N + i, soe);
        if (!last) {
            ldv<V>(tb + i, go);
            if (both) ldv<V>(tb + N + i, goe);
        }
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const float ds = consist_diff(sa0m1, sb0x, sb0e, both, z[j], so[j], soe[j]);
            const float dt = last ? 0.f : consist_diff(ga0m1, gb0x, gb0e, both, zs[j], go[j], goe[j]);
            r[j] = (ds - dt) - dz[j];
            acc += (double)r[j] * (double)r[j];
        }
        stv<V>(resid + b * N + i, r);
        if (target) {
            float tg[V];
#pragma unroll
            for (int j = 0; j < V; ++j) tg[j] = last ? zs[j] : x0_hat(ga0, gb0x, gb0e, both, zs[j], go[j], goe[j]);
            stv<V>(target + b * N + i, tg);
        }
    }
    acc = block_sum(acc, sh);
    if (threadIdx.x == 0) {
        const double om = (double)k[11];
        if (p.metric == 0) {
            loss[b] = (float)(om * (acc / (double)N));
            aux[b] = (float)(2.0 / (double)N);
        } else {
            const double q = sqrt(acc + p.c * p.c);
            loss[b] = (float)(om * (acc / (q + p.c)));
            aux[b] = (float)(1.0 / q);
        }
    }
}

// dout = gloss[b] * omega_b * aux[b] * resid * b0x (second half of a "both" student: * b0e)
template <int V>
__global__ void consist_loss_bwd_kernel(const float* resid, const float* coef, const float* gloss, const float* aux, int stype,
                                        float* dout, int n, long long N) {
#pragma clang fp contract(off)
    const long long total = (long long)n * N / V;
    const int Co = stype == OUT_BOTH ? 2 : 1;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const long long e = idx * V, b = e / N, i = e % N;
        const float* k = coef + CK * b;
        const float g = gloss[b] * k[11] * aux[b], bx = k[9], be = k[10];
        float r[V], d[V];
        ldv<V>(resid + e, r);
#pragma unroll
        for (int j = 0; j < V; ++j) d[j] = g * r[j] * bx;
        stv<V>(dout + b * Co * N + i, d);
        if (stype == OUT_BOTH) {
#pragma unroll
            for (int j = 0; j < V; ++j) d[j] = g * r[j] * be;
            stv<V>(dout + b * Co * N + N + i, d);
        }
    }
}

// e <- e + (1 - decay) (p - e), adamw_ema_kernel's expression, over every tensor of a module in ONE launch.  items: device table,
// 8 x int64 per tensor: {dst e, src p, count, 0, 0, 0, 0, first block}; blocks of 256 elements.  omd = 1 - decay; omd = 1 copies.
// A wave owns EMA_U consecutive blocks: one search of the table for the first, a walk for the rest; a full block whose two bases are
// 16-byte aligned moves as one dwordx4 per lane, any other as four coalesced dwords -- the same expression, the same bits.
enum { EMA_U = 4 };

__device__ __forceinline__ float ema_track(float e, float p, float omd) {
#pragma clang fp contract(off)
    return omd == 1.f ? p : e + omd * (p - e);
}

__global__ __launch_bounds__(256) void ema_track_batched_kernel(const long long* items, int n, long long total_blocks, float omd) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    long long blk = ((long long)blockIdx.x * 4 + wave) * EMA_U;
    if (blk >= total_blocks) return;
    int lo = 0, hi = n - 1;                                  // last item whose first block <= blk
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (items[8 * mid + 7] <= blk) lo = mid; else hi = mid - 1;
    }
    for (int u = 0; u < EMA_U && blk < total_blocks; ++u, ++blk) {
        while (lo + 1 < n && items[8 * (lo + 1) + 7] <= blk) ++lo;
        const long long* it = items + 8 * lo;
        const long long count = it[2], base = (blk - it[7]) * 256;
        float* dst = reinterpret_cast<float*>(it[0]) + base;
        const float* src = reinterpret_cast<const float*>(it[1]) + base;
        if (count - base >= 256 && ((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src)) & 15) == 0) {
            float e[4], p[4];
            ldv<4>(dst + 4 * lane, e);
            ldv<4>(src + 4 * lane, p);
#pragma unroll
            for (int j = 0; j < 4; ++j) e[j] = ema_track(e[j], p[j], omd);
            stv<4>(dst + 4 * lane, e);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int i = j * 64 + lane;
                if (base + i < count) dst[i] = ema_track(dst[i], src[i], omd);
            }
        }
    }
}

// ---- DPM-Solver++(2M) (Lu et al. 2022, data-prediction form): one reverse step of the probability-flow ODE in log-SNR time from the
// guided x0 prediction g of this step and the one of the step before (hist).  k[8] = {a0, b0x, b0e, c1, c2, c2*rho, w_guide, 0} with
// c1, c2 the DDIM weights of the step and rho = h / (2 h_prev); c2*rho = 0 gives the DDIM step, (c1, c2, c2*rho) = (0, 1, 0) the
// guided x0 prediction itself (the last row of a chain).  Evaluation order, every operation in fp32:
//   g = the guided PredX0 of the two branches (each clipped when asked)
//   xn  = c1*xt + c2*g + c2rho*(g - hist);   hist <- g;   xdup rows 2b, 2b+1 <- xn
// Each thread reads all it needs of its V elements before it writes any of them, so xn may alias xt.
struct SolverArgs { StepCommon s; float* hist; };

template <int V>
__global__ void solver_step_kernel(const SolverArgs p) {
    const StepCommon& s = p.s;
    const long long N = s.N, total = (long long)s.n * N / V;
    const float* k = coefs(s.c);
    const PredX0 f = pred_x0(s, k);
    const float c1 = k[3], c2 = k[4], c2r = k[5], w = k[6];
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const long long e = idx * V, b = e / N, i = e % N;
        float z[V], h[V], g[V], xn[V];
        ldv<V>(s.xt + e, z);
        ldv<V>(p.hist + e, h);
        guided<V>(s, b, i, w, z, f, g);
#pragma unroll
        for (int j = 0; j < V; ++j) xn[j] = solver_update(c1, c2, c2r, z[j], g[j], h[j]);
        stv<V>(p.hist + e, g);
        st_dup<V>(s.xn, s.xdup, b, N, i, xn);
    }
}

// ---- UniPC (Zhao et al. 2023, multistep, data-prediction form, B(h) = h or e^h - 1): one node of the predictor-corrector chain in ONE
// launch.  The network was called at the predicted state xt; its guided x0 prediction g first corrects the step that arrived at this
// node (the corrector and the predictor of a step share x_bar, so the corrected state is the predicted one plus differences of
// predictions: no further state image), then the predictor of the step that leaves starts from the corrected state, and the history
// of the last three predictions (h0 newest) shifts by one.  k[16] = {a0, b0x, b0e, w_guide, c1, c2, p1, p2, eg, e1, e2, 0...}:
// c1, c2 the DDIM weights of the leaving step, p_k = -alpha_next B rho^p_k / r_k, eg = -alpha B rho^c_p, e_k = -alpha B (rho^c_k -
// rho^p_k) / r_k (v_diffusion/unipc.py builds them).  Evaluation order, every operation in fp32:
//   g  = the guided PredX0 of the two branches (each clipped when asked)
//   xc = xt + eg*(g - h0) + e1*(h1 - h0) + e2*(h2 - h0)
//   xn = c1*xc + c2*g + p1*(h0 - g) + p2*(h1 - g)
//   h2 <- h1;  h1 <- h0;  h0 <- g;   xdup rows 2b, 2b+1 <- xn;   xc_out <- xc (optional)
// e = 0 (the first node, or no corrector) gives xc = xt; p2 = 0, p1 = -c2*rho the DPM-Solver++(2M) step; (c1, c2, p1, p2) = (0, 1, 0, 0)
// returns g.  Each thread reads all it needs of its V elements before it writes any of them, so xn may alias xt.
struct UnipcArgs { StepCommon s; float* h0; float* h1; float* h2; float* xc; };

template <int V>
__global__ void unipc_step_kernel(const UnipcArgs p) {
    const StepCommon& s = p.s;
    const long long N = s.N, total = (long long)s.n * N / V;
    const float* k = coefs(s.c);
    const PredX0 f = pred_x0(s, k);
    const float w = k[3], c1 = k[4], c2 = k[5], p1 = k[6], p2 = k[7], eg = k[8], e1 = k[9], e2 = k[10];
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const long long e = idx * V, b = e / N, i = e % N;
        float z[V], h0[V], h1[V], h2[V], g[V], xc[V], xn[V];
        ldv<V>(s.xt + e, z);
        ldv<V>(p.h0 + e, h0);
        ldv<V>(p.h1 + e, h1);
        ldv<V>(p.h2 + e, h2);
        guided<V>(s, b, i, w, z, f, g);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            xc[j] = unipc_correct(eg, e1, e2, z[j], g[j], h0[j], h1[j], h2[j]);
            xn[j] = unipc_predict(c1, c2, p1, p2, xc[j], g[j], h0[j], h1[j]);
        }
        stv<V>(p.h2 + e, h1);
        stv<V>(p.h1 + e, h0);
        stv<V>(p.h0 + e, g);
        if (p.xc) stv<V>(p.xc + e, xc);
        st_dup<V>(s.xn, s.xdup, b, N, i, xn);
    }
}

// ---- dynamic thresholding (Saharia et al. 2022, section 2.3) of the solver's guided x0 prediction: s = the element of rank r of |g|
// over the sample, clamped to [1, s_max]; g' = clamp(g, -s, s) / s.  The rank-r element is found by a radix select over the bit
// pattern of |g| (as unsigned integers the patterns order like the numbers, +Inf above every finite value, NaNs above +Inf): four
// passes of 8 bits from the top, each a 256-bin LDS histogram of the elements that still match the prefix, a scan for the bin that
// holds the rank, and a narrowing of prefix and rank.  Integer counting only: the result is exact and bitwise reproducible.
// ONE WORKGROUP OWNS ONE ROW from its first read to its last write, and nothing here can wait on another workgroup (no global
// counter, ticket, spin or atomic): every pass re-reads the row's inputs, which are at most a few hundred KB and stay in L2.
// The histogram exists in KTH_COPIES copies, lane l counting into copy l % KTH_COPIES with the copies one bank apart: the top bits
// of |g| fall into a handful of bins, and 64 lanes adding to one LDS word serialise.
enum { KTH_BINS = 256, KTH_COPIES = 8, KTH_PITCH = KTH_BINS + 1, KTH_THREADS = 1024 };

struct KthShared { uint32_t hist[KTH_COPIES * KTH_PITCH]; uint32_t prefix, rank; };

// bit pattern of the element of rank r (0-based, ascending) of |e_0|, ..., |e_{N-1}|, where prod(i, e) produces the elements
// [i, i + V) and must produce the same bits each time it is asked.  Called by every thread of the workgroup; r < N < 2^31.
template <int V, class Prod>
__device__ __forceinline__ uint32_t abs_kth_select(const Prod& prod, long long N, uint32_t r, KthShared& sh) {
    const int lane = threadIdx.x & 63;
    uint32_t prefix = 0, mask = 0;
#pragma unroll 1
    for (int shift = 24; shift >= 0; shift -= 8) {
        for (int t = threadIdx.x; t < KTH_COPIES * KTH_PITCH; t += blockDim.x) sh.hist[t] = 0;
        __syncthreads();
        uint32_t* mine = sh.hist + (threadIdx.x % KTH_COPIES) * KTH_PITCH;
        for (long long i = (long long)threadIdx.x * V; i < N; i += (long long)blockDim.x * V) {
            float e[V];
            prod(i, e);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const uint32_t key = __float_as_uint(e[j]) & 0x7fffffffu;
                if ((key & mask) == prefix) atomicAdd(mine + ((key >> shift) & (KTH_BINS - 1)), 1u);
            }
        }
        __syncthreads();
        if (threadIdx.x < 64) {                              // wave 0: lane l owns bins 4l .. 4l+3
            uint32_t c[4], tot = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                c[q] = 0;
#pragma unroll
                for (int u = 0; u < KTH_COPIES; ++u) c[q] += sh.hist[u * KTH_PITCH + 4 * lane + q];
                tot += c[q];
            }
            uint32_t upto = tot;                             // inclusive scan over the lanes
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t v = __shfl_up(upto, o, 64);
                if (lane >= o) upto += v;
            }
            const uint32_t before = upto - tot;
            if (r >= before && r < upto) {                   // true on exactly one lane: the counts sum to the elements still matching
                uint32_t rr = r - before;
                int q = 0;
#pragma unroll
                for (int t = 0; t < 3; ++t)
                    if (q == t && rr >= c[t]) { rr -= c[t]; q = t + 1; }
                sh.prefix = prefix | ((uint32_t)(4 * lane + q) << shift);
                sh.rank = rr;
            }
        }
        __syncthreads();
        prefix = sh.prefix; r = sh.rank; mask |= (uint32_t)(KTH_BINS - 1) << shift;
    }
    return prefix;
}

template <int V> struct RowProd {
    const float* row;
    __device__ __forceinline__ void operator()(long long i, float (&e)[V]) const { ldv<V>(row + i, e); }
};

template <int V>
__global__ __launch_bounds__(KTH_THREADS) void abs_kth_rows_kernel(const float* x, long long N, uint32_t r, float* kth) {
    __shared__ KthShared sh;
    const RowProd<V> prod = {x + (long long)blockIdx.x * N};
    const uint32_t key = abs_kth_select<V>(prod, N, r, sh);
    if (threadIdx.x == 0) kth[blockIdx.x] = __uint_as_float(key);
}

struct SolverDynArgs { StepCommon s; float* hist; uint32_t r; float s_max; float* s_out; };

// one workgroup per sample.  No thread writes before every thread has left the last selection pass (its closing barrier), and a
// thread reads all it needs of its V elements before it writes any of them, so xn may alias xt.
template <int V>
__global__ __launch_bounds__(KTH_THREADS) void solver_step_dyn_kernel(const SolverDynArgs p) {
    __shared__ KthShared sh;
    const StepCommon& s = p.s;
    const long long b = blockIdx.x, N = s.N;
    const float* k = coefs(s.c);
    const PredX0 f = {k[0], k[1], k[2], s.type == OUT_BOTH, false};       // unclipped: the threshold takes the clip's place
    const float c1 = k[3], c2 = k[4], c2r = k[5], w = k[6];
    // the state z and the unclipped guided x0 prediction g of elements [i, i + V): the same bits each time it is asked
    const auto eval = [&](long long i, float (&z)[V], float (&g)[V]) { ldv<V>(s.xt + b * N + i, z); guided<V>(s, b, i, w, z, f, g); };
    const auto prod = [&](long long i, float (&g)[V]) { float z[V]; eval(i, z, g); };
    const float s_raw = __uint_as_float(abs_kth_select<V>(prod, N, p.r, sh));
    const float t = s_raw != s_raw ? s_raw : fminf(fmaxf(s_raw, 1.f), p.s_max);       // a NaN of rank r stays one
    if (threadIdx.x == 0 && p.s_out) p.s_out[b] = t;
    for (long long i = (long long)threadIdx.x * V; i < N; i += (long long)blockDim.x * V) {
        float z[V], g[V], h[V], xn[V];
        eval(i, z, g);
        ldv<V>(p.hist + b * N + i, h);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            float c = g[j] < -t ? -t : (g[j] > t ? t : g[j]);                         // a NaN passes through
            if (t != 1.f) c = c / t;                                                  // IEEE division; c / 1 = c
            g[j] = c;
            xn[j] = solver_update(c1, c2, c2r, z[j], c, h[j]);
        }
        stv<V>(p.hist + b * N + i, g);
        st_dup<V>(s.xn, s.xdup, b, N, i, xn);
    }
}

// ---- RePaint inpainting (Lugmayr et al. 2022) in log-SNR terms: sample_step_kernel's reverse step for the unknown region, a draw from
// q(x_s | x_known) for the known one, and their merge by the mask, in one launch.  k[10] = sample_step_kernel's eight
// {a0, b0x, b0e, c1, c2, noise_scale, w_guide, c3} and {ak, bk}, the alpha and sigma of the state the step lands on.  Evaluation order,
// every operation in fp32:
//   v = the guided StepMean<fused> of the two branches;   u = v + noise_scale*noise  (when noise is given)
//   kn = ak*known + bk*knoise  (ak*known when knoise is null)
//   xn = m == 1 ? kn : m == 0 ? u : m*kn + (1 - m)*u;   xdup rows 2b, 2b+1 <- xn
// The two ends of the mask SELECT: a NaN or Inf of the branch not chosen does not reach xn.  full = the mask has C channels (else one,
// shared by the sample's channels: a vector of V elements must then lie inside one channel, HW % V == 0).
// Each thread reads all it needs of its V elements before it writes any of them, so xn may alias xt.
__device__ __forceinline__ float inp_merge(float m, float kn, float u) {
#pragma clang fp contract(off)
    return m == 1.f ? kn : (m == 0.f ? u : __builtin_fmaf(1.f - m, u, m * kn));
}

struct InpaintArgs { StepCommon s; const float* noise; const float* known; const float* mask; const float* knoise; int full; long long HW; };

template <int V>
__global__ void inpaint_step_kernel(const InpaintArgs p) {
    const StepCommon& s = p.s;
    const long long N = s.N, total = (long long)s.n * N / V;
    const float* k = coefs(s.c);
    const StepMean<true> f = step_mean<true>(s, k);
    const float nscale = k[5], w = k[6], ak = k[8], bk = k[9];
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const long long e = idx * V, b = e / N, i = e % N;
        float z[V], kw[V], m[V], nz[V], kz[V], v[V], xn[V];
        ldv<V>(s.xt + e, z);
        ldv<V>(p.known + e, kw);
        ldv<V>(p.mask + (p.full ? e : b * p.HW + i % p.HW), m);
        if (p.noise) ldv<V>(p.noise + e, nz);
        if (p.knoise) ldv<V>(p.knoise + e, kz);
        guided<V>(s, b, i, w, z, f, v);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            if (p.noise) v[j] = axpby(1.f, v[j], nscale, nz[j]);
            const float kn = p.knoise ? axpby(ak, kw[j], bk, kz[j]) : ak * kw[j];
            xn[j] = inp_merge(m[j], kn, v[j]);
        }
        st_dup<V>(s.xn, s.xdup, b, N, i, xn);
    }
}

// the forward transition q(x_t | x_s) of any length, xn = a*x + b*noise; xdup (optional) rows 2b, 2b+1 <- xn.  A thread reads its V
// elements before it writes them, so xn may alias x.
template <int V>
__global__ void forward_jump_kernel(const float* x, const float* noise, const float* k, float a, float b, float* xn, float* xdup, int n,
                                    long long N) {
    const long long total = (long long)n * N / V;
    if (k) { a = k[0]; b = k[1]; }                 // device-resident coefficients keep the launch HIP-graph replayable
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const long long e = idx * V, s = e / N, i = e % N;
        float z[V], nz[V], r[V];
        ldv<V>(x + e, z);
        ldv<V>(noise + e, nz);
#pragma unroll
        for (int j = 0; j < V; ++j) r[j] = axpby(a, z[j], b, nz[j]);
        stv<V>(xn + e, r);
        if (xdup) { stv<V>(xdup + 2 * s * N + i, r); stv<V>(xdup + (2 * s + 1) * N + i, r); }
    }
}

// ---- DDPM noise-space inversion (Huberman-Spiegelglas et al. 2024) in log-SNR terms: given the state xt = x_{i+1} and the network's
// output there, draw the next state from the image itself, xs = ak*x0 + bk*eps, and extract the noise map the ordinary reverse step
// would have needed to land on it, z = (xs - v)/noise_scale with v sample_step_kernel's guided mean.  k[10] = inpaint_step_kernel's ten.
// Evaluation order, every operation in fp32, v inpaint_step_kernel's guided StepMean<fused>:
//   xs = ak*x0 + bk*eps  (ak*x0 when eps is null): inpaint_step_kernel's known-region value, same expression, same bits
//   z  = (xs - v) / k[5]   one subtraction, one IEEE division;   xdup rows 2b, 2b+1 <- xs
// xs does not depend on xt or out: a NaN of the network stays in z.  Each thread reads all it needs of its V elements before it writes
// any of them, so xs may alias xt.
__device__ __forceinline__ float inv_extract(float xs, float v, float nscale) {
#pragma clang fp contract(off)
    return (xs - v) / nscale;
}

struct ExtractArgs { StepCommon s; const float* x0; const float* eps; float* z; };       // s.xn = xs

template <int V>
__global__ void noise_extract_kernel(const ExtractArgs p) {
    const StepCommon& s = p.s;
    const long long N = s.N, total = (long long)s.n * N / V;
    const float* k = coefs(s.c);
    const StepMean<true> f = step_mean<true>(s, k);
    const float nscale = k[5], w = k[6], ak = k[8], bk = k[9];
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const long long e = idx * V, b = e / N, i = e % N;
        float zt[V], im[V], ez[V], v[V], xs[V], zz[V];
        ldv<V>(s.xt + e, zt);
        ldv<V>(p.x0 + e, im);
        if (p.eps) ldv<V>(p.eps + e, ez);
        guided<V>(s, b, i, w, zt, f, v);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            xs[j] = p.eps ? axpby(ak, im[j], bk, ez[j]) : ak * im[j];
            zz[j] = inv_extract(xs[j], v[j], nscale);
        }
        stv<V>(p.z + e, zz);
        st_dup<V>(s.xn, s.xdup, b, N, i, xs);
    }
}

// ---- spherical interpolation of two latents per sample: out = wa*a + wb*b with (wa, wb) = (sin((1-f) w), sin(f w)) / sin w, w the
// angle between the rows.  ONE WORKGROUP OWNS ONE ROW, as in abs_kth_rows_kernel, and waits on no other.  Pass 1: thread t adds the
// products of its accesses t, t + 1024, ... (element order inside an access) to three fp64 sums <a,b>, |a|^2, |b|^2; the 64 lanes of a
// wave are added by a fixed butterfly and the 16 wave sums in wave order: no atomics, the same bits on every call.  Thread 0 forms the
// weights in fp64 and rounds each to fp32 once.  Pass 2 re-reads the rows (they stay in L2): out = fma(wb, b, wa*a), spelled out.
enum { SLERP_THREADS = 1024 };

template <int V>
__global__ __launch_bounds__(SLERP_THREADS) void slerp_rows_kernel(const float* a, const float* b, const float* frac, float frac_all,
                                                                   float* out, float* w_out, long long N) {
    __shared__ double sh[SLERP_THREADS / 64];
    __shared__ float wsh[2];
    const long long row = (long long)blockIdx.x * N;
    const float* ar = a + row;
    const float* br = b + row;
    double dab = 0.0, daa = 0.0, dbb = 0.0;
    for (long long i = (long long)threadIdx.x * V; i < N; i += (long long)SLERP_THREADS * V) {
        float x[V], y[V];
        ldv<V>(ar + i, x);
        ldv<V>(br + i, y);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const double xd = x[j], yd = y[j];
            dab = fma(xd, yd, dab); daa = fma(xd, xd, daa); dbb = fma(yd, yd, dbb);
        }
    }
    dab = block_sum(dab, sh); daa = block_sum(daa, sh); dbb = block_sum(dbb, sh);
    if (threadIdx.x == 0) {
        const double f = frac ? (double)frac[blockIdx.x] : (double)frac_all;
        double wa = 1.0 - f, wb = f;                         // the lerp weights: a zero row, or rows (anti)parallel to within sin w < 1e-6
        if (!(daa == 0.0) && !(dbb == 0.0)) {
            double c = dab / (sqrt(daa) * sqrt(dbb));
            c = c < -1.0 ? -1.0 : (c > 1.0 ? 1.0 : c);       // a NaN passes through, into this row's weights only
            const double om = acos(c), s = sin(om);
            if (!(s < 1e-6)) { wa = sin((1.0 - f) * om) / s; wb = sin(f * om) / s; }
        }
        wsh[0] = (float)wa; wsh[1] = (float)wb;
        if (w_out) { w_out[2 * blockIdx.x] = wsh[0]; w_out[2 * blockIdx.x + 1] = wsh[1]; }
    }
    __syncthreads();
    const float wa = wsh[0], wb = wsh[1];
    float* orow = out + row;
    for (long long i = (long long)threadIdx.x * V; i < N; i += (long long)SLERP_THREADS * V) {
        float x[V], y[V], r[V];
        ldv<V>(ar + i, x);
        ldv<V>(br + i, y);
#pragma unroll
        for (int j = 0; j < V; ++j) r[j] = axpby(wa, x[j], wb, y[j]);
        stv<V>(orow + i, r);
    }
}

// ---- Diffusion Posterior Sampling (Chung et al. 2023, Algorithm 1): every reverse step is followed by a gradient step on the
// measurement residual ||meas - A g(xt)||, g the guided (clipped) x0 prediction of the step.  Two launches around the network's input
// gradient.  dps_residual_kernel: r = meas - A g, sumsq[b] = sum r^2, and the cotangents of (1/2)||r||^2 with u = -A^T r and m the
// pass mask of the clip (PredX0::pass) -- unnormalised, the network's VJP is linear:
//   dout cond row (1 + w) m_c u, uncond row -w m_u u (without guidance m u), times b0x, and times b0e on the second half of "both";
//   dxt = a0 [(1 + w) m_c - w m_u] u (a0 m u): the path that does not go through the network;   x0hat (optional) = g.
// A: op 0 = M (.) g, the mask of par = 1 or C channels; op 1 = the mean over par x par blocks; op 2 = the mean over the channels.
// ONE WORKGROUP OWNS ONE SAMPLE and a thread one measurement element with its preimage (1, par^2 or C elements; the preimages tile the
// image, so every element of dout and dxt is written once): nothing but the sum crosses threads.  Each thread adds its r^2 in fp64 in
// element order, block_sum adds lanes and waves in a fixed order: no atomics, no workspace, the same bits on every call.
enum { DPS_MASK = 0, DPS_DOWN = 1, DPS_GRAY = 2 };

struct DpsResArgs {
    const float* xt; const float* out; const float* meas; const float* mask; Coefs c; int type, cfg, clip, op, par;
    float* dout; float* dxt; float* sumsq; float* x0hat; int C, H, W;
};

__device__ __forceinline__ float dps_apply(int op, float m, float sum, float cnt) {      // (A g) of one measurement element
#pragma clang fp contract(off)
    return op == DPS_MASK ? m * sum : sum / cnt;
}

__device__ __forceinline__ float dps_adjoint(int op, float m, float r, float cnt) {      // u = -(A^T r) of each element of its preimage
#pragma clang fp contract(off)
    return op == DPS_MASK ? -(m * r) : -(r / cnt);
}

struct DpsCot { float c, u, z; };      // the factors of u in the cond row, the uncond row and dxt

__device__ __forceinline__ DpsCot dps_cot(bool cfg, float w, float a0, float mc, float mu) {
#pragma clang fp contract(off)
    if (!cfg) return {mc, 0.f, a0 * mc};
    const float fc = (1.f + w) * mc, fu = -w * mu;
    return {fc, fu, a0 * (fc + fu)};
}

__device__ __forceinline__ float dps_mul(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}

__global__ __launch_bounds__(256) void dps_residual_kernel(const DpsResArgs p) {
    __shared__ double sh[4];
    const long long b = blockIdx.x, HW = (long long)p.H * p.W, N = p.C * HW;
    const float* k = p.c.k;
    const bool both = p.type == OUT_BOTH, cfg = p.cfg != 0;
    const PredX0 x0 = {k[0], k[1], k[2], both, p.clip != 0};
    const float a0 = k[0], b0x = k[1], b0e = k[2], w = k[6];
    const long long row = (both ? 2 : 1) * N;
    const float* zb = p.xt + b * N;
    const float* oc = p.out + b * (1 + p.cfg) * row;
    const float* ou = oc + row;
    float* dc = p.dout + b * (1 + p.cfg) * row;
    float* du = dc + row;
    const int op = p.op, f = op == DPS_DOWN ? p.par : 1, Wo = p.W / f, Ho = p.H / f;
    const int cnt = op == DPS_MASK ? 1 : (op == DPS_DOWN ? f * f : p.C);
    const long long M = op == DPS_MASK ? N : (op == DPS_DOWN ? (long long)p.C * Ho * Wo : HW);      // measurement elements of a sample
    // index in [0, N) of element q of the preimage of measurement element j
    auto elem = [&](long long j, int q) -> long long {
        if (op == DPS_MASK) return j;
        if (op == DPS_GRAY) return q * HW + j;
        const long long c = j / ((long long)Ho * Wo), r = j % ((long long)Ho * Wo), yo = r / Wo, xo = r % Wo;
        return c * HW + (yo * f + q / f) * p.W + xo * f + q % f;
    };
    // the guided prediction of element i and the pass masks of its two branches
    auto pred = [&](long long i, float& mc, float& mu) -> float {
        const float z = zb[i];
        const float pc = x0.raw(z, oc[i], both ? oc[N + i] : 0.f);
        mc = x0.pass(pc); mu = 0.f;
        float g = x0.clipped(pc);
        if (cfg) {
            const float pu = x0.raw(z, ou[i], both ? ou[N + i] : 0.f);
            mu = x0.pass(pu);
            g = guide(w, g, x0.clipped(pu));
        }
        return g;
    };
    double acc = 0.0;
    for (long long j = threadIdx.x; j < M; j += blockDim.x) {
        // (the up to 64 predictions of a preimage are added in fp64 and rounded once: r is a difference of two numbers of one size, and a
        // running fp32 sum's error would be most of it)
        double sum = 0.0;
        float g = 0.f, mc = 0.f, mu = 0.f;
        for (int q = 0; q < cnt; ++q) { g = pred(elem(j, q), mc, mu); sum += (double)g; }
        const float m = op == DPS_MASK ? p.mask[b * p.par * HW + (p.par == 1 ? j % HW : j)] : 1.f;
        const float r = p.meas[b * M + j] - dps_apply(op, m, (float)sum, (float)cnt);
        acc += (double)r * (double)r;
        const float u = dps_adjoint(op, m, r, (float)cnt);
        for (int q = 0; q < cnt; ++q) {
            const long long i = elem(j, q);
            if (cnt > 1) g = pred(i, mc, mu);
            const DpsCot t = dps_cot(cfg, w, a0, mc, mu);
            const float cc = dps_mul(t.c, u);
            dc[i] = dps_mul(cc, b0x);
            if (both) dc[N + i] = dps_mul(cc, b0e);
            if (cfg) {
                const float cu = dps_mul(t.u, u);
                du[i] = dps_mul(cu, b0x);
                if (both) du[N + i] = dps_mul(cu, b0e);
            }
            p.dxt[b * N + i] = dps_mul(t.z, u);
            if (p.x0hat) p.x0hat[b * N + i] = g;
        }
    }
    acc = block_sum(acc, sh);
    if (threadIdx.x == 0) p.sumsq[b] = (float)acc;
}

// ---- The blur operator of DPS (include/vdiff_blur.h): A g = the cross-correlation of every channel plane with ONE kh x kw kernel of
// taps, reflect boundary without repeating the edge (F.pad(mode="reflect") + F.conv2d, depthwise).  Its preimages overlap, so the
// "thread owns its preimage" split of dps_residual_kernel does not serve: a plane is staged in LDS and both A and A^T are stencils on it.
//   blur_apply    (A g)[y, x]   = sum_i sum_j tap[i, j] * g[rho_H(y + i - Rh), rho_W(x + j - Rw)],  i, j ascending
//   blur_adjoint  (A^T r)[y, x] = sum over p in pre_H(y), i, q in pre_W(x), j of tap[i, j] * r[p - i + Rh, q - j + Rw] where that lies in
//                 the plane; pre_n(y) = y, then -y if 1 <= y <= R, then 2(n - 1) - y if n - 1 - R <= y <= n - 2 (the positions of the
//                 padded axis that reflect onto y), in that order, i and j ascending inside -- the loops below ARE the order.
// Both accumulate in fp64 (fma) and round once, dps_apply's rule; the taps stand in LDS as doubles (every lane reads one address: a
// broadcast).  R <= n - 1 (the entries hold it) keeps rho inside the plane and the three preimages distinct.
enum { BLUR_THREADS = 1024 };

__device__ __forceinline__ int blur_reflect(int p, int n) {
    p = p < 0 ? -p : p;
    return min(p, 2 * (n - 1) - p);
}

struct BlurGeom { int kh, kw, H, W; };

__device__ __forceinline__ float blur_apply(const float* pl, const double* taps, const BlurGeom& q, int y, int x) {
    const int rh = q.kh >> 1, rw = q.kw >> 1;
    double acc = 0.0;
    for (int i = 0; i < q.kh; ++i) {
        const float* row = pl + blur_reflect(y + i - rh, q.H) * q.W;
        const double* tr = taps + i * q.kw;
        for (int j = 0; j < q.kw; ++j) acc = __builtin_fma(tr[j], (double)row[blur_reflect(x + j - rw, q.W)], acc);
    }
    return (float)acc;
}

// position s = 0, 1, 2 of pre_n(y); false when the set has no such entry
__device__ __forceinline__ bool blur_pre(int s, int y, int n, int r, int& p) {
    p = s == 0 ? y : (s == 1 ? -y : 2 * (n - 1) - y);
    return s == 0 || (s == 1 ? (y >= 1 && y <= r) : (y >= n - 1 - r && y <= n - 2));
}

__device__ __forceinline__ float blur_adjoint(const float* pl, const double* taps, const BlurGeom& q, int y, int x) {
    const int rh = q.kh >> 1, rw = q.kw >> 1;
    double acc = 0.0;
    for (int s = 0; s < 3; ++s) {
        int p;
        if (!blur_pre(s, y, q.H, rh, p)) continue;
        // the taps whose source row p - i + rh lies in the plane
        const int i0 = max(0, p + rh - q.H + 1), i1 = min(q.kh - 1, p + rh);
        for (int i = i0; i <= i1; ++i) {
            const float* row = pl + (p - i + rh) * q.W;
            const double* tr = taps + i * q.kw;
            for (int t = 0; t < 3; ++t) {
                int c;
                if (!blur_pre(t, x, q.W, rw, c)) continue;
                const int j0 = max(0, c + rw - q.W + 1), j1 = min(q.kw - 1, c + rw);
                for (int j = j0; j <= j1; ++j) acc = __builtin_fma(tr[j], (double)row[c - j + rw], acc);
            }
        }
    }
    return (float)acc;
}

enum { BLUR_KMAX = VDX_BLUR_KMAX, BLUR_PLANE_MAX = VDX_BLUR_PLANE_MAX };

__device__ __forceinline__ void blur_load_taps(const float* taps, double* sh, int count) {
    for (int i = threadIdx.x; i < count; i += blockDim.x) sh[i] = (double)taps[i];
}

// dps_blur_kernel: dps_residual_kernel's outputs for the blur operator.  ONE WORKGROUP OWNS ONE SAMPLE and walks its C channels; per
// channel three passes over the plane, element e = y W + x to thread e mod BLUR_THREADS in each:
//   1. g = the guided clipped prediction (dps_residual_kernel's pred: PredX0, guide) -> the LDS plane gp (and x0hat);          barrier
//   2. r = meas - blur_apply(gp); the thread's fp64 sum takes r^2; r -> the LDS plane rp;                                        barrier
//   3. u = -blur_adjoint(rp); dout, dxt from u exactly as dps_residual_kernel forms them (dps_cot, dps_mul; the pass masks are
//      recomputed from the inputs, as that kernel does for a preimage of more than one element);
// and a barrier before the next channel reuses the two planes.
// Every element of every output is written once, by one thread; sumsq is block_sum's fixed order: the same call gives the same bits.
struct DpsBlurArgs {
    const float* xt; const float* out; const float* meas; const float* taps; Coefs c; int type, cfg, clip;
    float* dout; float* dxt; float* sumsq; float* x0hat; int C; BlurGeom q;
};

__global__ __launch_bounds__(BLUR_THREADS) void dps_blur_kernel(const DpsBlurArgs p) {
    __shared__ double sh[BLUR_THREADS / 64];
    __shared__ double taps[BLUR_KMAX * BLUR_KMAX];
    __shared__ float gp[BLUR_PLANE_MAX], rp[BLUR_PLANE_MAX];
    const BlurGeom q = p.q;
    const int HW = q.H * q.W;
    const long long b = blockIdx.x, N = (long long)p.C * HW;
    const float* k = p.c.k;
    const bool both = p.type == OUT_BOTH, cfg = p.cfg != 0;
    const PredX0 x0 = {k[0], k[1], k[2], both, p.clip != 0};
    const float a0 = k[0], b0x = k[1], b0e = k[2], w = k[6];
    const long long row = (both ? 2 : 1) * N;
    const float* zb = p.xt + b * N;
    const float* oc = p.out + b * (1 + p.cfg) * row;
    const float* ou = oc + row;
    float* dc = p.dout + b * (1 + p.cfg) * row;
    float* du = dc + row;
    auto pred = [&](long long i, float& mc, float& mu) -> float {
        const float z = zb[i];
        const float pc = x0.raw(z, oc[i], both ? oc[N + i] : 0.f);
        mc = x0.pass(pc); mu = 0.f;
        float g = x0.clipped(pc);
        if (cfg) {
            const float pu = x0.raw(z, ou[i], both ? ou[N + i] : 0.f);
            mu = x0.pass(pu);
            g = guide(w, g, x0.clipped(pu));
        }
        return g;
    };
    blur_load_taps(p.taps, taps, q.kh * q.kw);
    double acc = 0.0;
    for (int c = 0; c < p.C; ++c) {
        const long long base = (long long)c * HW;
        for (int e = threadIdx.x; e < HW; e += BLUR_THREADS) {
            float mc, mu;
            const float g = pred(base + e, mc, mu);
            gp[e] = g;
            if (p.x0hat) p.x0hat[b * N + base + e] = g;
        }
        __syncthreads();
        for (int e = threadIdx.x; e < HW; e += BLUR_THREADS) {
            const float r = p.meas[b * N + base + e] - blur_apply(gp, taps, q, e / q.W, e % q.W);
            acc += (double)r * (double)r;
            rp[e] = r;
        }
        __syncthreads();
        for (int e = threadIdx.x; e < HW; e += BLUR_THREADS) {
            const long long i = base + e;
            const float u = -blur_adjoint(rp, taps, q, e / q.W, e % q.W);
            float mc, mu;
            pred(i, mc, mu);
            const DpsCot t = dps_cot(cfg, w, a0, mc, mu);
            const float cc = dps_mul(t.c, u);
            dc[i] = dps_mul(cc, b0x);
            if (both) dc[N + i] = dps_mul(cc, b0e);
            if (cfg) {
                const float cu = dps_mul(t.u, u);
                du[i] = dps_mul(cu, b0x);
                if (both) du[N + i] = dps_mul(cu, b0e);
            }
            p.dxt[b * N + i] = dps_mul(t.z, u);
        }
        __syncthreads();
    }
    acc = block_sum(acc, sh);
    if (threadIdx.x == 0) p.sumsq[b] = (float)acc;
}

// blur_planes_kernel: y = A x (adjoint = 0) or A^T x (1) of one plane per workgroup, by the two device functions above
__global__ __launch_bounds__(BLUR_THREADS) void blur_planes_kernel(const float* x, const float* tp, int adjoint, float* y, BlurGeom q) {
    __shared__ double taps[BLUR_KMAX * BLUR_KMAX];
    __shared__ float pl[BLUR_PLANE_MAX];
    const int HW = q.H * q.W;
    const long long base = (long long)blockIdx.x * HW;
    blur_load_taps(tp, taps, q.kh * q.kw);
    for (int e = threadIdx.x; e < HW; e += BLUR_THREADS) pl[e] = x[base + e];
    __syncthreads();
    for (int e = threadIdx.x; e < HW; e += BLUR_THREADS)
        y[base + e] = adjoint ? blur_adjoint(pl, taps, q, e / q.W, e % q.W) : blur_apply(pl, taps, q, e / q.W, e % q.W);
}

// dps_step_kernel: sample_step_kernel's row -- the same helpers: prediction, clip, guided mean_plain, last step, noise -- and then
//   xn -= zeta / sqrt(sumsq[b]) * (dxt[b] + dxin[2b] + dxin[2b+1])      (dxt[b] + dxin[b] without guidance)
// with dxin the network's input gradient of dps_residual_kernel's dout: the gradient of ||r|| itself, scaled by zeta.  The term is
// SELECTED: with zeta = 0 or sumsq[b] = 0 the row is sample_step_kernel's bit for bit and its dxin / dxt are never read; a sumsq[b]
// that is not finite makes that row NaN and no other.  Each thread reads all it needs of its V elements before it writes them, so xn
// may alias xt.
struct DpsStepArgs { StepCommon s; const float* noise; const float* dxin; const float* dxt; const float* sumsq; float zeta; };

__device__ __forceinline__ float dps_scale(float zeta, float ss) {
#pragma clang fp contract(off)
    return __builtin_isfinite(ss) ? zeta * (1.f / sqrtf(ss)) : __builtin_nanf("");     // (a negative ss: NaN from the root)
}

__device__ __forceinline__ float dps_correct(float v, float sc, float dz, float dc, float du, bool cfg) {
#pragma clang fp contract(off)
    const float d = cfg ? (dz + dc) + du : dz + dc;
    return __builtin_fmaf(-sc, d, v);
}

template <int V>
__global__ void dps_step_kernel(const DpsStepArgs p) {
    const StepCommon& s = p.s;
    const long long N = s.N, total = (long long)s.n * N / V;
    const float* k = coefs(s.c);
    const StepMean<false> f = step_mean<false>(s, k);
    const float k5 = k[5], w = k[6];
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const long long e = idx * V, b = e / N, i = e % N;
        float z[V], v[V];
        ldv<V>(s.xt + e, z);
        guided<V>(s, b, i, w, z, f, v);
        if (p.noise) {
            float nz[V];
            ldv<V>(p.noise + e, nz);
#pragma unroll
            for (int j = 0; j < V; ++j) v[j] = axpby(1.f, v[j], k5, nz[j]);
        }
        const float ss = p.sumsq[b];
        if (p.zeta != 0.f && ss != 0.f) {
            const float sc = dps_scale(p.zeta, ss);
            const float* dn = p.dxin + b * (1 + s.cfg) * N + i;
            float dz[V], dc[V], du[V] = {};
            ldv<V>(p.dxt + e, dz);
            ldv<V>(dn, dc);
            if (s.cfg) ldv<V>(dn + N, du);
#pragma unroll
            for (int j = 0; j < V; ++j) v[j] = dps_correct(v[j], sc, dz[j], dc[j], du[j], s.cfg != 0);
        }
        st_dup<V>(s.xn, s.xdup, b, N, i, v);
    }
}

// ---- Denoising Diffusion Null-space Model (Wang, Yu, Zhang 2023): the three operators of the DPS section have a closed-form
// pseudo-inverse, so the step's x0 prediction is corrected without a gradient: g_hat = g + lam * A^+(meas - A g) keeps the network's
// null-space part and takes the range-space part from the measurement.  ONE launch per reverse step: sample_step_kernel's value v (the
// same helpers: prediction, clip, guided mean_plain, last step, noise) and
//   xn = fma(cw, d, v),   d = A^+ r on the preimage,  r = meas_j - A g,  cw = lam on the last step and c2 * lam otherwise (host, rounded once)
// since v holds c2 * g.  A g is dps_apply's (the preimage summed in fp64, rounded once); d = r for the two means (A^+ spreads r over the
// preimage) and r / M for a mask element with M > 0.  SELECTED, not multiplied: with lam = 0 the row is sample_step_kernel's bit for bit
// (and without sumsq meas and mask are never read); a mask element with M = 0 has no measurement -- no correction, no share of sumsq,
// whatever meas holds there; with `exact` (mask, last step, lam = 1, no noise term) an element with M = 1 IS meas.
// The work split is dps_residual_kernel's: one workgroup owns one sample, a thread G adjacent measurement elements with their preimages
// (rows x LEN floats each: 1 x 1 mask, f x f blocks with LEN = f, C x 1 grey), so nothing but the optional sum crosses threads and a
// thread has read its whole preimage before it writes any of it (xn may alias xt; rows > 1 are read again, element by element, each
// before its own store).  G and LEN follow from the SHAPES alone -- G = 4 where the measurement rows are whole multiples of 4 -- and fix
// which thread adds which r^2 in which order; WIDE (every base 16-byte aligned) only turns the G * LEN floats of a row into dwordx2 /
// dwordx4 accesses: the same bits, sumsq included.
struct DdnmArgs {
    StepCommon s; const float* noise; const float* meas; const float* mask; float* sumsq; float lam, cw; int exact, op, par, C, H, W;
};

// VW = 1, 2 or 4 floats of a row: one access (ldv / stv) when WIDE, else element by element
template <int VW, bool WIDE> __device__ __forceinline__ void ld_row(const float* p, float (&r)[VW]) {
    if constexpr (WIDE) ldv<VW>(p, r);
    else {
#pragma unroll
        for (int j = 0; j < VW; ++j) r[j] = p[j];
    }
}

template <int VW, bool WIDE> __device__ __forceinline__ void st_row(float* p, const float (&r)[VW]) {
    if constexpr (WIDE) stv<VW>(p, r);
    else {
#pragma unroll
        for (int j = 0; j < VW; ++j) p[j] = r[j];
    }
}

// one sample's rows of the step's operands
struct DdnmRows { const float* z; const float* oc; const float* ou; int N; bool both, cfg; };

// elements [i, i + VW) of the sample: g = the guided clipped prediction (dps_residual_kernel's pred), v = sample_step_kernel's guided mean
template <int VW, bool WIDE>
__device__ __forceinline__ void ddnm_row(const DdnmRows& t, const StepMean<false>& f, float w, int i, float (&g)[VW], float (&v)[VW]) {
    float z[VW], o[VW], oe[VW] = {};
    ld_row<VW, WIDE>(t.z + i, z);
    ld_row<VW, WIDE>(t.oc + i, o);
    if (t.both) ld_row<VW, WIDE>(t.oc + t.N + i, oe);
#pragma unroll
    for (int j = 0; j < VW; ++j) { g[j] = f.x0(z[j], o[j], oe[j]); v[j] = f.of(z[j], g[j], o[j]); }
    if (t.cfg) {
        ld_row<VW, WIDE>(t.ou + i, o);
        if (t.both) ld_row<VW, WIDE>(t.ou + t.N + i, oe);
#pragma unroll
        for (int j = 0; j < VW; ++j) {
            const float pu = f.x0(z[j], o[j], oe[j]);
            v[j] = guide(w, v[j], f.of(z[j], pu, o[j]));
            g[j] = guide(w, g[j], pu);
        }
    }
}

__device__ __forceinline__ float ddnm_pinv(int op, float m, float r) {      // (A^+ r) of each element of the preimage; m > 0
#pragma clang fp contract(off)
    return op == DPS_MASK ? r / m : r;
}

__device__ __forceinline__ float ddnm_sub(float y, float ag) {
#pragma clang fp contract(off)
    return y - ag;
}

template <int OP, int G, int LEN, bool WIDE>
__global__ __launch_bounds__(256) void ddnm_step_kernel(const DdnmArgs p) {
    // a thread's row of G * LEN floats goes in pieces of at most 4 (LEN = 8: two), left to right: the order of the fp64 sum
    constexpr int VW = G * LEN > 4 ? 4 : G * LEN, PIECES = G * LEN / VW;
    __shared__ double sh[4];
    const StepCommon& s = p.s;
    const float* k = s.c.k;
    const StepMean<false> f = step_mean<false>(s, k);
    const float k5 = k[5], w = k[6];
    // (offsets inside one sample are 32-bit -- the entry refuses C*H*W >= 2^31 -- and only the sample's bases 64-bit)
    const long long b = blockIdx.x;
    const int N = (int)s.N, HW = p.H * p.W;
    const int Wo = p.W / LEN, HoWo = p.H / LEN * Wo;                                          // (LEN > 1: down-sampling by LEN)
    const int rows = OP == DPS_MASK ? 1 : (OP == DPS_DOWN ? LEN : p.C);
    const int stride = OP == DPS_DOWN ? p.W : HW;
    const float cnt = (float)(rows * LEN);
    const int M = OP == DPS_MASK ? N : (OP == DPS_DOWN ? p.C * HoWo : HW);        // measurement elements of a sample
    const bool corr = p.lam != 0.f, need = corr || p.sumsq != nullptr, once = need && rows == 1;
    const bool mask_wide = WIDE && (p.par != 1 || HW % G == 0);              // (a one-channel mask: a group may straddle two channels)
    const DdnmRows in = {s.xt + b * s.N, s.out + b * (1 + s.cfg) * s.row, s.out + (b * (1 + s.cfg) + 1) * s.row, N, s.type == OUT_BOTH,
                         s.cfg != 0};
    const float* nb = p.noise ? p.noise + b * s.N : nullptr;
    const float* yb = p.meas + b * M;
    const float* mb = OP == DPS_MASK ? p.mask + b * p.par * (long long)HW : nullptr;
    float* xb = s.xn + b * s.N;
    float* db = s.xdup ? s.xdup + 2 * b * s.N : nullptr;
    double acc = 0.0;
    for (int t = threadIdx.x; t < M / G; t += blockDim.x) {
        const int j0 = t * G;
        int i0 = j0;
        if constexpr (OP == DPS_DOWN) {
            const int c = j0 / HoWo, r = j0 % HoWo, yo = r / Wo, xo = r % Wo;
            i0 = c * HW + yo * LEN * p.W + xo * LEN;
        }
        float g[VW], v[VW], y[G] = {}, m[G] = {}, d[G] = {};                  // (m stays 0 where nothing is taken: no lane mask kept)
        if (need) {
            double sum[G] = {};
#pragma unroll 1
            for (int q = 0; q < rows * PIECES; ++q) {
                ddnm_row<VW, WIDE>(in, f, w, i0 + q / PIECES * stride + q % PIECES * VW, g, v);
#pragma unroll
                for (int e = 0; e < VW; ++e) sum[G == 1 ? 0 : e / LEN] += (double)g[e];
            }
            ld_row<G, WIDE>(yb + j0, y);
#pragma unroll
            for (int e = 0; e < G; ++e) m[e] = 1.f;
            if constexpr (OP == DPS_MASK) {
                if (mask_wide) ld_row<G, WIDE>(mb + (p.par == 1 ? j0 % HW : j0), m);
                else {
#pragma unroll
                    for (int e = 0; e < G; ++e) m[e] = mb[p.par == 1 ? (j0 + e) % HW : j0 + e];
                }
            }
#pragma unroll
            for (int e = 0; e < G; ++e) {
                if (m[e] > 0.f) {
                    const float r = ddnm_sub(y[e], dps_apply(OP, m[e], (float)sum[e], cnt));
                    acc += (double)r * (double)r;
                    d[e] = ddnm_pinv(OP, m[e], r);
                }
            }
        }
#pragma unroll 1
        for (int q = 0; q < rows * PIECES; ++q) {
            const int i = i0 + q / PIECES * stride + q % PIECES * VW;
            if (!once) ddnm_row<VW, WIDE>(in, f, w, i, g, v);
            if (nb) {
                float nz[VW];
                ld_row<VW, WIDE>(nb + i, nz);
#pragma unroll
                for (int e = 0; e < VW; ++e) v[e] = axpby(1.f, v[e], k5, nz[e]);
            }
#pragma unroll
            for (int e = 0; e < VW; ++e) {
                const int u = G == 1 ? 0 : e / LEN;
                if (corr && m[u] > 0.f) v[e] = (p.exact && m[u] == 1.f) ? y[u] : __builtin_fmaf(p.cw, d[u], v[e]);
            }
            st_row<VW, WIDE>(xb + i, v);
            if (db) { st_row<VW, WIDE>(db + i, v); st_row<VW, WIDE>(db + N + i, v); }
        }
    }
    if (p.sumsq) {                                                           // (uniform over the workgroup)
        acc = block_sum(acc, sh);
        if (threadIdx.x == 0) p.sumsq[b] = (float)acc;
    }
}

// ---- host side of the entries below
template <typename... P> inline bool all_aligned16(P... ps) { return (vd_aligned16(ps) && ...); }

#define VD_TRY(call) do { if (const int rc_ = (call)) return rc_; } while (0)

// the dwordx4 instantiation when wide (the element count is a multiple of 4 and every base 16-byte aligned), else the scalar one:
// grid-stride kernels over total elements, and kernels whose workgroup of `threads` owns one of n rows
template <class K, class... A> inline void launch_elems(K k4, K k1, bool wide, long long total, void* stream, const A&... a) {
    hipLaunchKernelGGL(wide ? k4 : k1, dim3(grid_for(wide ? total / 4 : total)), dim3(256), 0, (hipStream_t)stream, a...);
}

template <class K, class... A> inline void launch_rows(K k4, K k1, bool wide, int n, int threads, void* stream, const A&... a) {
    hipLaunchKernelGGL(wide ? k4 : k1, dim3(n), dim3(threads), 0, (hipStream_t)stream, a...);
}

// count coefficients as host floats k (copied into the kernel argument) or as a device pointer k_dev, never both
inline int set_coefs(const char* who, Coefs& c, const float* k, const float* k_dev, int count) {
    VD_REQUIRE((k != nullptr) != (k_dev != nullptr), "%s: pass the coefficients either as host k or as device k_dev", who);
    c = {};
    for (int i = 0; i < count; ++i) c.k[i] = k ? k[i] : 0.f;
    c.kdev = k_dev;
    return 0;
}

inline StepCommon step_common(const float* xt, const float* out, int type, int cfg, int last, int clip, float* xn, float* xdup, int n,
                              int C, int HW) {
    StepCommon s = {};
    s.xt = xt; s.out = out; s.type = type; s.cfg = cfg ? 1 : 0; s.last = last ? 1 : 0; s.clip = clip ? 1 : 0;
    s.xn = xn; s.xdup = xdup; s.n = n; s.N = (long long)C * HW;
    s.row = (type == OUT_BOTH ? 2 : 1) * s.N;
    return s;
}

inline LossArgs loss_args(const float* x0, const float* eps, const float* xt, const float* out, const float* logsnr, int type, int rw, int n,
                          int C, int HW) {
    return {x0, eps, xt, out, logsnr, type, rw, n, C, (long long)HW};
}

inline BpdArgs bpd_args(const float* x0, const float* xt, const float* out, const float* coef, int type, int clip, int n, int C, int HW) {
    return {x0, xt, out, coef, type, clip ? 1 : 0, n, C, (long long)HW};
}

// The refusals the entries share, each in one wording; the first that applies is the one reported.  A refused call has launched nothing.
// ptrs = the buffers the kernel dereferences for these arguments are all given
inline int args_given(const char* who, int type, bool ptrs) {
    VD_REQUIRE(type >= 0 && type <= 3, "%s: bad model_out_type %d", who, type);
    VD_REQUIRE(ptrs, "%s: null pointer", who);
    return 0;
}

inline int not_empty(const char* who, int n, int C, int HW) {
    VD_REQUIRE(n > 0 && C > 0 && HW > 0, "%s: empty batch or image (n=%d, C=%d, HW=%d)", who, n, C, HW);
    return 0;
}

inline int args_checks(const char* who, int type, bool ptrs, int n, int C, int HW) {          // both
    VD_TRY(args_given(who, type, ptrs));
    return not_empty(who, n, C, HW);
}

// the mse and hybrid loss entries: the reweighting too, and the reference's shape rule
inline int loss_checks(const char* who, int type, int rw, bool ptrs) {
    VD_REQUIRE(rw >= 0 && rw <= 3, "%s: bad reweight %d", who, rw);
    VD_TRY(args_given(who, type, ptrs));
    VD_REQUIRE(!(type == OUT_BOTH && rw != RW_SNR_TRUNC), "%s: 'both' output needs snr_trunc (reference shape rule)", who);
    return 0;
}

// the step entries: the coefficients too
inline int step_checks(const char* who, StepCommon& s, const float* k, const float* k_dev, int count, bool ptrs, int C, int HW) {
    VD_TRY(set_coefs(who, s.c, k, k_dev, count));
    return args_checks(who, s.type, ptrs, s.n, C, HW);
}

inline int dup_is_guided(const char* who, const StepCommon& s) {
    VD_REQUIRE(!s.xdup || s.cfg, "%s: the duplicated state is the guided network's input (cfg = 1)", who);
    return 0;
}

}  // namespace

extern "C" int vd_q_sample(const float* x0, const float* eps, const float* logsnr, float* xt, int32_t n, int32_t C,
                           int32_t HW, void* stream) {
    VD_TRY(args_given("vd_q_sample", OUT_V, x0 && eps && logsnr && xt));          // (no output type here)
    const long long chw = (long long)C * HW;                                     // an empty call launches one idle workgroup
    hipLaunchKernelGGL(q_sample_kernel, dim3(grid_for(n * chw)), dim3(256), 0, (hipStream_t)stream, x0, eps, logsnr, xt,
                       (long long)n, chw);
    VD_LAUNCH_CHECK("q_sample_kernel");
    return 0;
}

extern "C" int vd_loss_fwd(const float* x0, const float* eps, const float* xt, const float* out, const float* logsnr,
                           int32_t type, int32_t rw, float* loss, float* aux, int32_t n, int32_t C, int32_t HW, void* stream) {
    VD_TRY(loss_checks("vd_loss_fwd", type, rw, x0 && eps && xt && out && logsnr && loss && aux));
    VD_TRY(not_empty("vd_loss_fwd", n, C, HW));
    hipLaunchKernelGGL(loss_fwd_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, loss_args(x0, eps, xt, out, logsnr, type, rw, n, C, HW),
                       loss, aux);
    VD_LAUNCH_CHECK("loss_fwd_kernel");
    return 0;
}

extern "C" int vd_loss_bwd(const float* x0, const float* eps, const float* xt, const float* out, const float* logsnr,
                           const float* aux, const float* gloss, int32_t type, int32_t rw, float* dout, int32_t n, int32_t C,
                           int32_t HW, void* stream) {
    VD_TRY(loss_checks("vd_loss_bwd", type, rw, x0 && eps && xt && out && logsnr && aux && gloss && dout));
    hipLaunchKernelGGL(loss_bwd_kernel, dim3(grid_for((long long)n * C * HW)), dim3(256), 0, (hipStream_t)stream,
                       loss_args(x0, eps, xt, out, logsnr, type, rw, n, C, HW), aux, gloss, dout);
    VD_LAUNCH_CHECK("loss_bwd_kernel");
    return 0;
}

// (xdup is accepted without guidance, and an empty batch is a no-op: no dup_is_guided, no not_empty)
extern "C" int vd_sample_step(const float* xt, const float* out, const float* noise, const float* k, const float* k_dev,
                              int32_t type, int32_t cfg, int32_t last_step, int32_t clip, float* xn, float* xdup, int32_t n,
                              int32_t C, int32_t HW, void* stream) {
    StepArgs p = {step_common(xt, out, type, cfg, last_step, clip, xn, xdup, n, C, HW), noise};
    VD_TRY(set_coefs("vd_sample_step", p.s.c, k, k_dev, 8));
    VD_TRY(args_given("vd_sample_step", type, xt && out && xn));
    VD_REQUIRE(noise != nullptr || k_dev != nullptr || k[5] == 0.f, "vd_sample_step: noise required when the noise scale is non-zero");
    launch_elems(sample_step_kernel<4, false>, sample_step_kernel<1, false>, p.s.N % 4 == 0 && all_aligned16(xt, out, noise, xn, xdup),
                 n * p.s.N, stream, p);
    VD_LAUNCH_CHECK("sample_step_kernel");
    return 0;
}

extern "C" int vd_bpd_terms(const float* x0, const float* xt, const float* out, const float* coef, int32_t type, int32_t clip,
                            float* kl, float* nll, float* pred, float* mse, int32_t n, int32_t C, int32_t HW, void* stream) {
    VD_TRY(args_checks("vd_bpd_terms", type, x0 && xt && out && coef && kl && nll, n, C, HW));
    hipLaunchKernelGGL(bpd_terms_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, bpd_args(x0, xt, out, coef, type, clip, n, C, HW), kl,
                       nll, pred, mse);
    VD_LAUNCH_CHECK("bpd_terms_kernel");
    return 0;
}

extern "C" int vd_bpd_bwd(const float* x0, const float* xt, const float* out, const float* coef, const float* use_kl,
                          const float* gloss, int32_t type, int32_t clip, float* dout, int32_t n, int32_t C, int32_t HW,
                          void* stream) {
    VD_TRY(args_given("vd_bpd_bwd", type, x0 && xt && out && coef && use_kl && gloss && dout));
    hipLaunchKernelGGL(bpd_bwd_kernel, dim3(grid_for((long long)n * C * HW)), dim3(256), 0, (hipStream_t)stream,
                       bpd_args(x0, xt, out, coef, type, clip, n, C, HW), use_kl, gloss, dout);
    VD_LAUNCH_CHECK("bpd_bwd_kernel");
    return 0;
}

extern "C" int vd_bpd_terms_lv(const float* x0, const float* xt, const float* out, const float* coef, int32_t type, int32_t clip,
                               float* kl, float* nll, float* pred, float* mse, int32_t n, int32_t C, int32_t HW, void* stream) {
    VD_TRY(args_checks("vd_bpd_terms_lv", type, x0 && xt && out && coef && kl && nll, n, C, HW));
    hipLaunchKernelGGL(bpd_terms_lv_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, bpd_args(x0, xt, out, coef, type, clip, n, C, HW),
                       kl, nll, pred, mse);
    VD_LAUNCH_CHECK("bpd_terms_lv_kernel");
    return 0;
}

extern "C" int vd_bpd_bwd_lv(const float* x0, const float* xt, const float* out, const float* coef, const float* use_kl,
                             const float* gloss, int32_t type, int32_t clip, int32_t mean_grad, float* dout, int32_t n, int32_t C,
                             int32_t HW, void* stream) {
    VD_TRY(args_checks("vd_bpd_bwd_lv", type, x0 && xt && out && coef && use_kl && gloss && dout, n, C, HW));
    hipLaunchKernelGGL(bpd_bwd_lv_kernel, dim3(grid_for((long long)n * C * HW)), dim3(256), 0, (hipStream_t)stream,
                       bpd_args(x0, xt, out, coef, type, clip, n, C, HW), use_kl, gloss, (int)(mean_grad ? 1 : 0), dout);
    VD_LAUNCH_CHECK("bpd_bwd_lv_kernel");
    return 0;
}

extern "C" int vd_hybrid_loss_fwd(const float* x0, const float* eps, const float* xt, const float* out, const float* logsnr,
                                  const float* coef, const float* use_kl, int32_t type, int32_t rw, float vlb_weight, float* loss,
                                  float* aux, int32_t n, int32_t C, int32_t HW, void* stream) {
    VD_TRY(loss_checks("vd_hybrid_loss_fwd", type, rw, x0 && eps && xt && out && logsnr && coef && use_kl && loss && aux));
    VD_TRY(not_empty("vd_hybrid_loss_fwd", n, C, HW));
    const LossArgs p = loss_args(x0, eps, xt, out, logsnr, type, rw, n, C, HW);
    hipLaunchKernelGGL(hybrid_fwd_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, p, coef, use_kl, vlb_weight, loss, aux);
    VD_LAUNCH_CHECK("hybrid_fwd_kernel");
    return 0;
}

extern "C" int vd_hybrid_loss_bwd(const float* x0, const float* eps, const float* xt, const float* out, const float* logsnr,
                                  const float* coef, const float* use_kl, const float* aux, const float* gloss, int32_t type, int32_t rw,
                                  float vlb_weight, float* dout, int32_t n, int32_t C, int32_t HW, void* stream) {
    VD_TRY(loss_checks("vd_hybrid_loss_bwd", type, rw, x0 && eps && xt && out && logsnr && coef && use_kl && aux && gloss && dout));
    VD_TRY(not_empty("vd_hybrid_loss_bwd", n, C, HW));
    const LossArgs p = loss_args(x0, eps, xt, out, logsnr, type, rw, n, C, HW);
    hipLaunchKernelGGL(hybrid_bwd_kernel, dim3(grid_for((long long)n * C * HW)), dim3(256), 0, (hipStream_t)stream, p, coef, use_kl,
                       vlb_weight, aux, gloss, dout);
    VD_LAUNCH_CHECK("hybrid_bwd_kernel");
    return 0;
}

extern "C" int vd_sample_step_lv(const float* xt, const float* out, const float* noise, const float* k, int32_t type, int32_t cfg,
                                 int32_t last_step, int32_t clip, float* xn, float* xdup, int32_t n, int32_t C, int32_t HW, void* stream) {
    StepArgs p = {step_common(xt, out, type, cfg, last_step, clip, xn, xdup, n, C, HW), noise};
    VD_REQUIRE(k != nullptr, "vd_sample_step_lv: the ten coefficients are host floats (no device form)");
    VD_TRY(step_checks("vd_sample_step_lv", p.s, k, nullptr, 10, xt && out && xn, C, HW));
    VD_TRY(dup_is_guided("vd_sample_step_lv", p.s));
    p.s.row += p.s.N;                                         // the variance channels follow the prediction channels
    launch_elems(sample_step_kernel<4, true>, sample_step_kernel<1, true>, p.s.N % 4 == 0 && all_aligned16(xt, out, noise, xn, xdup),
                 n * p.s.N, stream, p);
    VD_LAUNCH_CHECK("sample_step_kernel (learned variances)");
    return 0;
}

extern "C" int vd_distill_mid(const float* zt, const float* out, const float* coef, int32_t teacher_type, int32_t cfg, int32_t clip,
                              float* xhat, float* dhat, float* zmid, float* zdup, int32_t n, int32_t C, int32_t HW, void* stream) {
    VD_TRY(args_checks("vd_distill_mid", teacher_type, zt && out && coef && xhat && dhat && zmid, n, C, HW));
    VD_REQUIRE(!zdup || cfg, "vd_distill_mid: the duplicated state is the guided teacher's input (cfg = 1)");
    const long long N = (long long)C * HW;
    DistillMidArgs p = {zt, out, coef, teacher_type, cfg ? 1 : 0, clip ? 1 : 0, xhat, dhat, zmid, zdup, n, N};
    launch_elems(distill_mid_kernel<4>, distill_mid_kernel<1>, N % 4 == 0 && all_aligned16(zt, out, xhat, dhat, zmid, zdup), n * N, stream, p);
    VD_LAUNCH_CHECK("distill_mid_kernel");
    return 0;
}

extern "C" int vd_distill_loss_fwd(const float* xhat, const float* dhat, const float* zmid, const float* teacher_out, const float* zt,
                                   const float* student_out, const float* coef, int32_t teacher_type, int32_t student_type, int32_t cfg,
                                   int32_t clip, float* loss, float* resid, float* xtilde, int32_t n, int32_t C, int32_t HW,
                                   void* stream) {
    VD_TRY(args_given("vd_distill_loss_fwd", teacher_type, true));
    VD_TRY(args_checks("vd_distill_loss_fwd", student_type,
                       dhat && zmid && teacher_out && zt && student_out && coef && loss && resid && (xhat || !xtilde), n, C, HW));
    const long long N = (long long)C * HW;
    DistillLossArgs p = {xhat, dhat, zmid, teacher_out, zt, student_out, coef, teacher_type, student_type, cfg ? 1 : 0, clip ? 1 : 0, n, N};
    launch_rows(distill_loss_fwd_kernel<4>, distill_loss_fwd_kernel<1>,
                N % 4 == 0 && all_aligned16(xhat, dhat, zmid, teacher_out, zt, student_out, resid, xtilde), n, 256, stream, p, loss, resid, xtilde);
    VD_LAUNCH_CHECK("distill_loss_fwd_kernel");
    return 0;
}

extern "C" int vd_distill_loss_bwd(const float* resid, const float* coef, const float* gloss, int32_t student_type, float* dout,
                                   int32_t n, int32_t C, int32_t HW, void* stream) {
    VD_TRY(args_checks("vd_distill_loss_bwd", student_type, resid && coef && gloss && dout, n, C, HW));
    const long long N = (long long)C * HW;
    launch_elems(distill_loss_bwd_kernel<4>, distill_loss_bwd_kernel<1>, N % 4 == 0 && all_aligned16(resid, dout), n * N, stream, resid, coef,
                 gloss, (int)student_type, dout, (int)n, N);
    VD_LAUNCH_CHECK("distill_loss_bwd_kernel");
    return 0;
}

extern "C" int vd_consist_mid(const float* zt, const float* out, const float* coef, int32_t teacher_type, int32_t cfg, int32_t clip,
                              float* zs, float* dz, float* xhat, int32_t n, int32_t C, int32_t HW, void* stream) {
    VD_TRY(args_checks("vd_consist_mid", teacher_type, zt && out && coef && zs && dz, n, C, HW));
    const long long N = (long long)C * HW;
    ConsistMidArgs p = {zt, out, coef, teacher_type, cfg ? 1 : 0, clip ? 1 : 0, zs, dz, xhat, n, N};
    launch_elems(consist_mid_kernel<4>, consist_mid_kernel<1>, N % 4 == 0 && all_aligned16(zt, out, zs, dz, xhat), n * N, stream, p);
    VD_LAUNCH_CHECK("consist_mid_kernel");
    return 0;
}

extern "C" int vd_consist_pair(const float* x0, const float* eps, const float* coef, float* zt, float* zs, float* dz, int32_t n,
                               int32_t C, int32_t HW, void* stream) {
    VD_TRY(args_checks("vd_consist_pair", OUT_V, x0 && eps && coef && zt && zs && dz, n, C, HW));          // (no output type here)
    const long long N = (long long)C * HW;
    launch_elems(consist_pair_kernel<4>, consist_pair_kernel<1>, N % 4 == 0 && all_aligned16(x0, eps, zt, zs, dz), n * N, stream, x0, eps,
                 coef, zt, zs, dz, (int)n, N);
    VD_LAUNCH_CHECK("consist_pair_kernel");
    return 0;
}

extern "C" int vd_consist_loss_fwd(const float* zt, const float* zs, const float* dz, const float* student_out, const float* target_out,
                                   const float* coef, int32_t out_type, int32_t metric, double huber_c, float* loss, float* resid,
                                   float* aux, float* target, int32_t n, int32_t C, int32_t HW, void* stream) {
    VD_REQUIRE(metric == 0 || (metric == 1 && huber_c > 0.0), "vd_consist_loss_fwd: metric must be 0 (l2) or 1 (huber, c > 0)");
    VD_TRY(args_checks("vd_consist_loss_fwd", out_type, zt && zs && dz && student_out && target_out && coef && loss && resid && aux, n, C, HW));
    const long long N = (long long)C * HW;
    ConsistLossArgs p = {zt, zs, dz, student_out, target_out, coef, out_type, metric, huber_c, n, N};
    launch_rows(consist_loss_fwd_kernel<4>, consist_loss_fwd_kernel<1>,
                N % 4 == 0 && all_aligned16(zt, zs, dz, student_out, target_out, resid, target), n, 256, stream, p, loss, resid, aux, target);
    VD_LAUNCH_CHECK("consist_loss_fwd_kernel");
    return 0;
}

extern "C" int vd_consist_loss_bwd(const float* resid, const float* coef, const float* gloss, const float* aux, int32_t out_type,
                                   float* dout, int32_t n, int32_t C, int32_t HW, void* stream) {
    VD_TRY(args_checks("vd_consist_loss_bwd", out_type, resid && coef && gloss && aux && dout, n, C, HW));
    const long long N = (long long)C * HW;
    launch_elems(consist_loss_bwd_kernel<4>, consist_loss_bwd_kernel<1>, N % 4 == 0 && all_aligned16(resid, dout), n * N, stream, resid, coef,
                 gloss, aux, (int)out_type, dout, (int)n, N);
    VD_LAUNCH_CHECK("consist_loss_bwd_kernel");
    return 0;
}

extern "C" int vd_ema_track_batched(const int64_t* items_dev, int32_t n, int64_t total_blocks, double decay, void* stream) {
    VD_REQUIRE(items_dev && n > 0 && total_blocks > 0 && total_blocks < (1LL << 31), "vd_ema_track_batched: bad table");
    VD_REQUIRE(decay >= 0.0 && decay <= 1.0, "vd_ema_track_batched: decay must lie in [0, 1]");
    const float omd = (float)(1.0 - decay);                  // rounded once, as a tensor expression rounds its scalar
    if (omd == 0.f) return 0;                                // decay = 1: the target stays as it is, whatever the source holds
    const long long per_group = 4 * EMA_U;                  // blocks per workgroup of four waves
    hipLaunchKernelGGL(ema_track_batched_kernel, dim3((unsigned)((total_blocks + per_group - 1) / per_group)), dim3(256), 0,
                       (hipStream_t)stream, reinterpret_cast<const long long*>(items_dev), (int)n, (long long)total_blocks, omd);
    VD_LAUNCH_CHECK("ema_track_batched_kernel");
    return 0;
}

extern "C" int vd_solver_step(const float* xt, const float* out, float* hist, const float* k, const float* k_dev, int32_t type,
                              int32_t cfg, int32_t clip, float* xn, float* xdup, int32_t n, int32_t C, int32_t HW, void* stream) {
    SolverArgs p = {step_common(xt, out, type, cfg, 0, clip, xn, xdup, n, C, HW), hist};
    VD_TRY(step_checks("vd_solver_step", p.s, k, k_dev, 8, xt && out && hist && xn, C, HW));
    VD_TRY(dup_is_guided("vd_solver_step", p.s));
    VD_REQUIRE(hist != xt && hist != xn, "vd_solver_step: hist is a buffer of its own");
    launch_elems(solver_step_kernel<4>, solver_step_kernel<1>, p.s.N % 4 == 0 && all_aligned16(xt, out, hist, xn, xdup), n * p.s.N, stream, p);
    VD_LAUNCH_CHECK("solver_step_kernel");
    return 0;
}

extern "C" int vd_unipc_step(const float* xt, const float* out, float* h0, float* h1, float* h2, const float* k, const float* k_dev,
                             int32_t type, int32_t cfg, int32_t clip, float* xn, float* xdup, float* xc_out, int32_t n, int32_t C, int32_t HW,
                             void* stream) {
    UnipcArgs p = {step_common(xt, out, type, cfg, 0, clip, xn, xdup, n, C, HW), h0, h1, h2, xc_out};
    VD_TRY(step_checks("vd_unipc_step", p.s, k, k_dev, 16, xt && out && h0 && h1 && h2 && xn, C, HW));
    VD_TRY(dup_is_guided("vd_unipc_step", p.s));
    const float* const hs[3] = {h0, h1, h2};
    for (const float* h : hs)
        VD_REQUIRE(h != xt && h != xn && h != xc_out, "vd_unipc_step: each history image is a buffer of its own");
    VD_REQUIRE(h0 != h1 && h0 != h2 && h1 != h2, "vd_unipc_step: each history image is a buffer of its own");
    VD_REQUIRE(!xc_out || (xc_out != xt && xc_out != xn), "vd_unipc_step: xc_out is a buffer of its own");
    launch_elems(unipc_step_kernel<4>, unipc_step_kernel<1>, p.s.N % 4 == 0 && all_aligned16(xt, out, h0, h1, h2, xn, xdup, xc_out),
                 n * p.s.N, stream, p);
    VD_LAUNCH_CHECK("unipc_step_kernel");
    return 0;
}

extern "C" int vd_abs_kth_rows(const float* x, int32_t n, int64_t N, int64_t r, float* kth, void* stream) {
    VD_REQUIRE(x && kth, "vd_abs_kth_rows: null pointer");
    VD_REQUIRE(n > 0 && N > 0, "vd_abs_kth_rows: empty batch or row (n=%d, N=%lld)", n, (long long)N);
    VD_REQUIRE(N <= VD_KTH_MAX_ROW, "vd_abs_kth_rows: rows of at most %lld elements (N=%lld)", (long long)VD_KTH_MAX_ROW, (long long)N);
    VD_REQUIRE(r >= 0 && r < N, "vd_abs_kth_rows: rank %lld outside [0, %lld)", (long long)r, (long long)N);
    launch_rows(abs_kth_rows_kernel<4>, abs_kth_rows_kernel<1>, N % 4 == 0 && vd_aligned16(x), n, KTH_THREADS, stream, x, (long long)N,
                (uint32_t)r, kth);
    VD_LAUNCH_CHECK("abs_kth_rows_kernel");
    return 0;
}

extern "C" int vd_solver_step_dyn(const float* xt, const float* out, float* hist, const float* k, const float* k_dev, int32_t type,
                                  int32_t cfg, int64_t r, float s_max, float* s_out, float* xn, float* xdup, int32_t n, int32_t C,
                                  int32_t HW, void* stream) {
    SolverDynArgs p = {step_common(xt, out, type, cfg, 0, 0, xn, xdup, n, C, HW), hist, (uint32_t)r, s_max, s_out};
    VD_TRY(step_checks("vd_solver_step_dyn", p.s, k, k_dev, 8, xt && out && hist && xn, C, HW));
    VD_TRY(dup_is_guided("vd_solver_step_dyn", p.s));
    VD_REQUIRE(hist != xt && hist != xn, "vd_solver_step_dyn: hist is a buffer of its own");
    VD_REQUIRE(s_max >= 1.f, "vd_solver_step_dyn: s_max must be >= 1 (+Inf for no cap), got %g", (double)s_max);
    const long long N = p.s.N;
    VD_REQUIRE(N <= VD_KTH_MAX_ROW, "vd_solver_step_dyn: images of at most %lld elements (C*HW=%lld)", (long long)VD_KTH_MAX_ROW, N);
    VD_REQUIRE(r >= 0 && r < N, "vd_solver_step_dyn: rank %lld outside [0, %lld)", (long long)r, N);
    launch_rows(solver_step_dyn_kernel<4>, solver_step_dyn_kernel<1>, N % 4 == 0 && all_aligned16(xt, out, hist, xn, xdup), n, KTH_THREADS,
                stream, p);
    VD_LAUNCH_CHECK("solver_step_dyn_kernel");
    return 0;
}

extern "C" int vd_inpaint_step(const float* xt, const float* out, const float* noise, const float* known, const float* mask,
                               const float* knoise, const float* k, const float* k_dev, int32_t type, int32_t cfg, int32_t last_step,
                               int32_t clip, int32_t mask_c, float* xn, float* xdup, int32_t n, int32_t C, int32_t HW, void* stream) {
    InpaintArgs p = {step_common(xt, out, type, cfg, last_step, clip, xn, xdup, n, C, HW), noise, known, mask, knoise, mask_c == C ? 1 : 0, HW};
    VD_TRY(step_checks("vd_inpaint_step", p.s, k, k_dev, 10, xt && out && known && mask && xn, C, HW));
    VD_REQUIRE(mask_c == 1 || mask_c == C, "vd_inpaint_step: mask_c must be 1 or C (mask_c=%d, C=%d)", mask_c, C);
    VD_TRY(dup_is_guided("vd_inpaint_step", p.s));
    VD_REQUIRE(noise != nullptr || k_dev != nullptr || k[5] == 0.f, "vd_inpaint_step: noise required when the noise scale is non-zero");
    VD_REQUIRE(knoise != nullptr || k_dev != nullptr || k[9] == 0.f, "vd_inpaint_step: knoise required when bk is non-zero");
    // a one-channel mask is indexed per channel: a vector must not straddle two channels
    launch_elems(inpaint_step_kernel<4>, inpaint_step_kernel<1>,
                 p.s.N % 4 == 0 && (p.full || HW % 4 == 0) && all_aligned16(xt, out, noise, known, mask, knoise, xn, xdup), n * p.s.N, stream, p);
    VD_LAUNCH_CHECK("inpaint_step_kernel");
    return 0;
}

extern "C" int vd_forward_jump(const float* x, const float* noise, const float* k, const float* k_dev, float* xn, float* xdup, int32_t n,
                               int64_t N, void* stream) {
    Coefs c;
    VD_TRY(set_coefs("vd_forward_jump", c, k, k_dev, 2));
    VD_REQUIRE(x && noise && xn, "vd_forward_jump: null pointer");
    VD_REQUIRE(n > 0 && N > 0, "vd_forward_jump: empty batch or image (n=%d, N=%lld)", n, (long long)N);
    launch_elems(forward_jump_kernel<4>, forward_jump_kernel<1>, N % 4 == 0 && all_aligned16(x, noise, xn, xdup), n * (long long)N, stream, x,
                 noise, k_dev, c.k[0], c.k[1], xn, xdup, (int)n, (long long)N);
    VD_LAUNCH_CHECK("forward_jump_kernel");
    return 0;
}

extern "C" int vd_noise_extract(const float* xt, const float* out, const float* x0, const float* eps, const float* k, const float* k_dev,
                                int32_t type, int32_t cfg, int32_t last_step, int32_t clip, float* xs, float* z, float* xdup, int32_t n,
                                int32_t C, int32_t HW, void* stream) {
    ExtractArgs p = {step_common(xt, out, type, cfg, last_step, clip, xs, xdup, n, C, HW), x0, eps, z};
    VD_TRY(step_checks("vd_noise_extract", p.s, k, k_dev, 10, xt && out && x0 && xs && z, C, HW));
    VD_TRY(dup_is_guided("vd_noise_extract", p.s));
    VD_REQUIRE(z != xs && z != xt && z != x0 && z != eps && xs != x0 && xs != eps, "vd_noise_extract: z is a buffer of its own, and xs may alias xt only");
    VD_REQUIRE(k_dev != nullptr || (std::isfinite(k[5]) && k[5] != 0.f), "vd_noise_extract: the noise scale k[5] must be finite and non-zero, got %g",
               (double)k[5]);
    VD_REQUIRE(eps != nullptr || k_dev != nullptr || k[9] == 0.f, "vd_noise_extract: eps required when bk is non-zero");
    launch_elems(noise_extract_kernel<4>, noise_extract_kernel<1>, p.s.N % 4 == 0 && all_aligned16(xt, out, x0, eps, xs, z, xdup), n * p.s.N,
                 stream, p);
    VD_LAUNCH_CHECK("noise_extract_kernel");
    return 0;
}

extern "C" int vd_slerp_rows(const float* a, const float* b, const float* frac, const float* frac_dev, float* out, float* w_out, int32_t n,
                             int64_t N, void* stream) {
    VD_REQUIRE((frac != nullptr) != (frac_dev != nullptr), "vd_slerp_rows: pass the fraction either as one host float or as n device floats");
    VD_REQUIRE(a && b && out, "vd_slerp_rows: null pointer");
    VD_REQUIRE(n > 0 && N > 0, "vd_slerp_rows: empty batch or row (n=%d, N=%lld)", n, (long long)N);
    VD_REQUIRE(out != a && out != b, "vd_slerp_rows: out may alias neither input (the rows are read twice)");
    const float f = frac ? frac[0] : 0.f;
    launch_rows(slerp_rows_kernel<4>, slerp_rows_kernel<1>, N % 4 == 0 && all_aligned16(a, b, out), n, SLERP_THREADS, stream, a, b, frac_dev, f,
                out, w_out, (long long)N);
    VD_LAUNCH_CHECK("slerp_rows_kernel");
    return 0;
}

// (Diffusion Posterior Sampling.  No device-resident coefficients: the chain has no captured-graph form)
extern "C" int vd_dps_residual(const float* xt, const float* out, const float* meas, const float* mask, const float* k, int32_t type,
                               int32_t cfg, int32_t clip, int32_t op, int32_t par, float* dout, float* dxt, float* sumsq, float* x0hat,
                               int32_t n, int32_t C, int32_t H, int32_t W, void* stream) {
    DpsResArgs p = {xt, out, meas, mask, {}, type, cfg ? 1 : 0, clip ? 1 : 0, op, par, dout, dxt, sumsq, x0hat, C, H, W};
    VD_REQUIRE(k != nullptr, "vd_dps_residual: null pointer");
    VD_TRY(set_coefs("vd_dps_residual", p.c, k, nullptr, 8));
    VD_REQUIRE(op >= DPS_MASK && op <= DPS_GRAY, "vd_dps_residual: bad op %d", op);
    VD_TRY(args_given("vd_dps_residual", type, xt && out && meas && dout && dxt && sumsq && (op != DPS_MASK || mask)));
    VD_REQUIRE(n > 0 && C > 0 && H > 0 && W > 0, "vd_dps_residual: empty batch or image (n=%d, C=%d, H=%d, W=%d)", n, C, H, W);
    VD_REQUIRE(op != DPS_MASK || par == 1 || par == C, "vd_dps_residual: the mask has 1 or C = %d channels, got %d", C, par);
    VD_REQUIRE(op != DPS_DOWN || ((par == 2 || par == 4 || par == 8) && H % par == 0 && W % par == 0),
               "vd_dps_residual: down-sampling by %d of a %d x %d image (the factor is 2, 4 or 8 and divides both sides)", par, H, W);
    hipLaunchKernelGGL(dps_residual_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, p);
    VD_LAUNCH_CHECK("dps_residual_kernel");
    return 0;
}

extern "C" int vd_dps_step(const float* xt, const float* out, const float* noise, const float* dxin, const float* dxt, const float* sumsq,
                           const float* k, float zeta, int32_t type, int32_t cfg, int32_t last_step, int32_t clip, float* xn, float* xdup,
                           int32_t n, int32_t C, int32_t HW, void* stream) {
    DpsStepArgs p = {step_common(xt, out, type, cfg, last_step, clip, xn, xdup, n, C, HW), noise, dxin, dxt, sumsq, zeta};
    VD_REQUIRE(k != nullptr, "vd_dps_step: null pointer");
    VD_TRY(step_checks("vd_dps_step", p.s, k, nullptr, 8, xt && out && dxin && dxt && sumsq && xn, C, HW));
    VD_REQUIRE(noise != nullptr || k[5] == 0.f, "vd_dps_step: noise required when the noise scale is non-zero");
    launch_elems(dps_step_kernel<4>, dps_step_kernel<1>, p.s.N % 4 == 0 && all_aligned16(xt, out, noise, dxin, dxt, xn, xdup), n * p.s.N, stream,
                 p);
    VD_LAUNCH_CHECK("dps_step_kernel");
    return 0;
}

// (the blur operator, include/vdiff_blur.h.)  What both entries refuse of the kernel and the plane, after their own pointers and counts
static int blur_checks(const char* who, int kh, int kw, int H, int W) {
    VD_REQUIRE(kh >= 1 && kh <= BLUR_KMAX && kw >= 1 && kw <= BLUR_KMAX && (kh & 1) && (kw & 1),
               "%s: a kernel of %d x %d taps (both sides are odd and at most %d)", who, kh, kw, (int)BLUR_KMAX);
    VD_REQUIRE(kh / 2 <= H - 1 && kw / 2 <= W - 1, "%s: the radii %d, %d of the kernel do not fit a %d x %d plane (at most H - 1, W - 1)", who,
               kh / 2, kw / 2, H, W);
    VD_REQUIRE((long long)H * W <= BLUR_PLANE_MAX, "%s: a plane of %d x %d is over the bound of %d elements", who, H, W, (int)BLUR_PLANE_MAX);
    return 0;
}

extern "C" int vdx_dps_residual_blur(const float* xt, const float* out, const float* meas, const float* taps, const float* k, int32_t type,
                                     int32_t cfg, int32_t clip, int32_t kh, int32_t kw, float* dout, float* dxt, float* sumsq, float* x0hat,
                                     int32_t n, int32_t C, int32_t H, int32_t W, void* stream) {
    DpsBlurArgs p = {xt, out, meas, taps, {}, type, cfg ? 1 : 0, clip ? 1 : 0, dout, dxt, sumsq, x0hat, C, {kh, kw, H, W}};
    VD_REQUIRE(k != nullptr, "vdx_dps_residual_blur: null pointer");
    VD_TRY(set_coefs("vdx_dps_residual_blur", p.c, k, nullptr, 8));
    VD_TRY(args_given("vdx_dps_residual_blur", type, xt && out && meas && taps && dout && dxt && sumsq));
    VD_REQUIRE(n > 0 && C > 0 && H > 0 && W > 0, "vdx_dps_residual_blur: empty batch or image (n=%d, C=%d, H=%d, W=%d)", n, C, H, W);
    VD_TRY(blur_checks("vdx_dps_residual_blur", kh, kw, H, W));
    hipLaunchKernelGGL(dps_blur_kernel, dim3(n), dim3(BLUR_THREADS), 0, (hipStream_t)stream, p);
    VD_LAUNCH_CHECK("dps_blur_kernel");
    return 0;
}

extern "C" int vdx_blur_planes(const float* x, const float* taps, int32_t kh, int32_t kw, int32_t adjoint, float* y, int32_t planes,
                               int32_t H, int32_t W, void* stream) {
    VD_REQUIRE(x && taps && y, "vdx_blur_planes: null pointer");
    VD_REQUIRE(adjoint == 0 || adjoint == 1, "vdx_blur_planes: adjoint is 0 (A) or 1 (A^T), got %d", adjoint);
    VD_REQUIRE(planes > 0 && H > 0 && W > 0, "vdx_blur_planes: empty batch or image (planes=%d, H=%d, W=%d)", planes, H, W);
    VD_TRY(blur_checks("vdx_blur_planes", kh, kw, H, W));
    hipLaunchKernelGGL(blur_planes_kernel, dim3(planes), dim3(BLUR_THREADS), 0, (hipStream_t)stream, x, taps, adjoint, y, BlurGeom{kh, kw, H, W});
    VD_LAUNCH_CHECK("blur_planes_kernel");
    return 0;
}

// (DDNM.  Host coefficients only, as the DPS entries: the chain has no captured-graph form)
extern "C" int vd_ddnm_step(const float* xt, const float* out, const float* noise, const float* meas, const float* mask, const float* k,
                            float lam, int32_t type, int32_t cfg, int32_t last_step, int32_t clip, int32_t op, int32_t par, float* xn,
                            float* xdup, float* sumsq, int32_t n, int32_t C, int32_t H, int32_t W, void* stream) {
    VD_REQUIRE(k != nullptr, "vd_ddnm_step: null pointer");
    VD_REQUIRE(op >= DPS_MASK && op <= DPS_GRAY, "vd_ddnm_step: bad op %d", op);
    VD_TRY(args_given("vd_ddnm_step", type, xt && out && meas && xn && (op != DPS_MASK || mask)));
    VD_REQUIRE(n > 0 && C > 0 && H > 0 && W > 0, "vd_ddnm_step: empty batch or image (n=%d, C=%d, H=%d, W=%d)", n, C, H, W);
    VD_REQUIRE(op != DPS_MASK || par == 1 || par == C, "vd_ddnm_step: the mask has 1 or C = %d channels, got %d", C, par);
    VD_REQUIRE(op != DPS_DOWN || ((par == 2 || par == 4 || par == 8) && H % par == 0 && W % par == 0),
               "vd_ddnm_step: down-sampling by %d of a %d x %d image (the factor is 2, 4 or 8 and divides both sides)", par, H, W);
    VD_REQUIRE((long long)C * H * W * (type == OUT_BOTH ? 2 : 1) <= 0x7fffffffLL, "vd_ddnm_step: a sample of %d x %d x %d is too large", C, H, W);
    VD_REQUIRE(noise != nullptr || k[5] == 0.f, "vd_ddnm_step: noise required when the noise scale is non-zero");
    const bool last = last_step != 0;
    DdnmArgs p = {step_common(xt, out, type, cfg, last_step, clip, xn, xdup, n, C, H * W), noise, meas, mask, sumsq, lam,
                  last ? lam : k[4] * lam, op == DPS_MASK && last && lam == 1.f && (!noise || k[5] == 0.f), op, par, C, H, W};
    VD_TRY(set_coefs("vd_ddnm_step", p.s.c, k, nullptr, 8));
    const bool wide = all_aligned16(xt, out, noise, meas, mask, xn, xdup);
    // the form follows from the shapes (G = 4 where a sample's measurement rows are whole multiples of 4), the access width from the bases
    const bool four = (op == DPS_MASK ? p.s.N : (long long)H * W) % 4 == 0;
    if (op == DPS_DOWN) {
        if (par == 2) launch_rows(ddnm_step_kernel<DPS_DOWN, 1, 2, true>, ddnm_step_kernel<DPS_DOWN, 1, 2, false>, wide, n, 256, stream, p);
        else if (par == 4) launch_rows(ddnm_step_kernel<DPS_DOWN, 1, 4, true>, ddnm_step_kernel<DPS_DOWN, 1, 4, false>, wide, n, 256, stream, p);
        else launch_rows(ddnm_step_kernel<DPS_DOWN, 1, 8, true>, ddnm_step_kernel<DPS_DOWN, 1, 8, false>, wide, n, 256, stream, p);
    } else if (op == DPS_MASK) {
        if (four) launch_rows(ddnm_step_kernel<DPS_MASK, 4, 1, true>, ddnm_step_kernel<DPS_MASK, 4, 1, false>, wide, n, 256, stream, p);
        else launch_rows(ddnm_step_kernel<DPS_MASK, 1, 1, false>, ddnm_step_kernel<DPS_MASK, 1, 1, false>, false, n, 256, stream, p);
    } else {
        if (four) launch_rows(ddnm_step_kernel<DPS_GRAY, 4, 1, true>, ddnm_step_kernel<DPS_GRAY, 4, 1, false>, wide, n, 256, stream, p);
        else launch_rows(ddnm_step_kernel<DPS_GRAY, 1, 1, false>, ddnm_step_kernel<DPS_GRAY, 1, 1, false>, false, n, 256, stream, p);
    }
    VD_LAUNCH_CHECK("ddnm_step_kernel");
    return 0;
}
