// optim.hip -- optimizer tail as multi-tensor passes over FLAT fp32 buffers:
// global-norm clip (nn.utils.clip_grad_norm_, train_utils.py:161) + AdamW (train.py:158) + EMA (utils.py:144-149)
#include "common.h"
#include "../../include/vdiff_phema.h"

namespace {

__global__ __launch_bounds__(256) void sumsq_partial_kernel(const float* g, long long n, float* part) {
    __shared__ float sh[4];
    float s = 0.f;
    const long long n4 = n >> 2;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
        const f32x4 v = reinterpret_cast<const f32x4*>(g)[i];
        s += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) { const float v = g[(n4 << 2) + threadIdx.x]; s += v * v; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}
__global__ void sumsq_final_kernel(const float* part, int nb, float* out) {
    __shared__ double sh[256];
    double s = 0.0;
    for (int i = threadIdx.x; i < nb; i += blockDim.x) s += (double)part[i];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o]; __syncthreads(); }
    if (threadIdx.x == 0) out[0] = (float)sh[0];
}

// [r_lo, r_hi): an index range with its own treatment this step (the class-embedding tensors, reference unet.py:207-215):
//   r_mode 1: the range received NO gradient (class-conditional network called with y = None: the reference leaves .grad None
//             and torch.optim.AdamW skips the parameter -- no moment decay, no weight decay, no update, step not advanced);
//             p, m, v stay untouched, the EMA shadow still follows p (utils.py:144-149 walks every parameter);
//   r_mode 2: the range is updated with its own bias corrections r_bc1 / r_bc2 (its per-parameter step count lags the rest).
//   r_mode 3: decided ON THE DEVICE (vd_adamw_ema_flagged): r_flag[0] > 0 -> as r_mode 2 with the bias corrections of step count
//             r_steps[0] + 1 (1 - beta^k evaluated here in double), else as r_mode 1; cls_step_advance_kernel then advances r_steps[0].
//             In data-parallel runs the flag is one extra slot behind the flat gradient buffer, summed over ranks by the LAST bucket's
//             all-reduce (trainer.FlatState): whether the class embedding received a gradient is one decision for all replicas, made
//             without a collective of its own and without any host reading it.
// every operand of the update is streamed once: non-temporal accesses (VD_OPT_NT=0: plain; same-box A/B tests/probe/r04_pass15.sh:
// 404-409 vs 439-442 us for the 243 MB CIFAR buffers, 5.4 vs 5.0 TB/s)
#ifndef VD_OPT_NT
#define VD_OPT_NT 1
#endif
__device__ __forceinline__ float ld1(const float* p) {
#if VD_OPT_NT
    return __builtin_nontemporal_load(p);
#else
    return *p;
#endif
}
__device__ __forceinline__ void st1(float* p, float v) {
#if VD_OPT_NT
    __builtin_nontemporal_store(v, p);
#else
    *p = v;
#endif
}
__global__ void adamw_ema_kernel(float* p, const float* g, float* m, float* v, float* ema, long long n, const float* gnorm_sq,
                                 float max_norm, float lr, float b1, float b2, float omb1, float omb2, float eps, float wd, float bc1,
                                 float bc2, float omd, long long r_lo, long long r_hi, int r_mode, float r_bc1, float r_bc2,
                                 const float* r_flag, const int* r_steps, double r_beta1, double r_beta2) {
    if (r_mode == 3) {
        if (r_flag[0] > 0.f) {
            const double kc = (double)(r_steps[0] + 1);
            r_bc1 = (float)(1.0 - pow(r_beta1, kc));
            r_bc2 = (float)(1.0 - pow(r_beta2, kc));
            r_mode = 2;
        } else {
            r_mode = 1;
        }
    }
    float clip = 1.f;
    if (gnorm_sq && max_norm > 0.f) {
        const float c = max_norm / (sqrtf(gnorm_sq[0]) + 1e-6f);          // torch clip_grad_norm_
        clip = c < 1.f ? c : 1.f;
    }
    const float step = lr / bc1, rs2 = 1.f / sqrtf(bc2);
    const float r_step = lr / r_bc1, r_rs2 = 1.f / sqrtf(r_bc2);
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const bool in_r = r_mode != 0 && i >= r_lo && i < r_hi;
        float pi = ld1(p + i);
        if (!(in_r && r_mode == 1)) {
            const float gi = ld1(g + i) * clip;
            pi *= 1.f - lr * wd;
            const float mi = b1 * ld1(m + i) + omb1 * gi;
            const float vi = b2 * ld1(v + i) + omb2 * gi * gi;
            pi -= (in_r ? r_step : step) * mi / (sqrtf(vi) * (in_r ? r_rs2 : rs2) + eps);
            st1(p + i, pi); st1(m + i, mi); st1(v + i, vi);
        }
        if (ema) { const float e = ld1(ema + i); st1(ema + i, e + omd * (pi - e)); }
    }
}

__global__ void cls_step_advance_kernel(const float* r_flag, int* r_steps) {
    if (r_flag[0] > 0.f) r_steps[0] += 1;
}

// The same tail with NP power-function EMA shadows (Karras et al. 2024, section 3.5: beta_t = (1 - 1/t)^(gamma + 1)) behind the classic
// one: e_k += r_k (p_new - e_k), r_k = 1 - beta_t formed in double on the host and rounded to fp32 once.  A rate of exactly 1 (t = 1)
// SELECTS p_new and leaves the shadow unread.  The update of p, m, v and ema repeats adamw_ema_kernel's lines so that that kernel's device
// code stays what it was (FINDINGS: ISA compared); each power shadow adds one dword load and one dword store per element to the one pass.
constexpr int PEMA_MAX = 4;
template <int NP> struct PemaArgs { float* e[NP]; float r[NP]; };
template <int NP>
__global__ void adamw_emas_kernel(float* p, const float* g, float* m, float* v, float* ema, long long n, const float* gnorm_sq,
                                  float max_norm, float lr, float b1, float b2, float omb1, float omb2, float eps, float wd, float bc1,
                                  float bc2, float omd, long long r_lo, long long r_hi, int r_mode, float r_bc1, float r_bc2,
                                  const float* r_flag, const int* r_steps, double r_beta1, double r_beta2, const PemaArgs<NP> pe) {
    if (r_mode == 3) {
        if (r_flag[0] > 0.f) {
            const double kc = (double)(r_steps[0] + 1);
            r_bc1 = (float)(1.0 - pow(r_beta1, kc));
            r_bc2 = (float)(1.0 - pow(r_beta2, kc));
            r_mode = 2;
        } else {
            r_mode = 1;
        }
    }
    float clip = 1.f;
    if (gnorm_sq && max_norm > 0.f) {
        const float c = max_norm / (sqrtf(gnorm_sq[0]) + 1e-6f);          // torch clip_grad_norm_
        clip = c < 1.f ? c : 1.f;
    }
    const float step = lr / bc1, rs2 = 1.f / sqrtf(bc2);
    const float r_step = lr / r_bc1, r_rs2 = 1.f / sqrtf(r_bc2);
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const bool in_r = r_mode != 0 && i >= r_lo && i < r_hi;
        float pi = ld1(p + i);
        if (!(in_r && r_mode == 1)) {
            const float gi = ld1(g + i) * clip;
            pi *= 1.f - lr * wd;
            const float mi = b1 * ld1(m + i) + omb1 * gi;
            const float vi = b2 * ld1(v + i) + omb2 * gi * gi;
            pi -= (in_r ? r_step : step) * mi / (sqrtf(vi) * (in_r ? r_rs2 : rs2) + eps);
            st1(p + i, pi); st1(m + i, mi); st1(v + i, vi);
        }
        if (ema) { const float e = ld1(ema + i); st1(ema + i, e + omd * (pi - e)); }
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            if (pe.r[k] == 1.f) {
                st1(pe.e[k] + i, pi);
            } else {
                const float e = ld1(pe.e[k] + i);
                st1(pe.e[k] + i, e + pe.r[k] * (pi - e));
            }
        }
    }
}

// out = (float) s, s = acc + sum_j w[j] src_j in fp64, one fma per source in ascending j: the post-hoc EMA reconstruction's combination
// of snapshots.  The sources and weights travel in the kernel arguments (the host has dropped the sources of weight 0).  V: four
// elements per lane through 16-byte accesses (every base 16-byte aligned), the n & 3 tail elements one lane each; else one element per
// lane.  The per-element chain is the same either way: the same bits.
constexpr int COMBINE_MAX = 32;
struct CombineArgs { const float* s[COMBINE_MAX]; double w[COMBINE_MAX]; };
typedef double f64x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ double combine_one(const CombineArgs& a, int k, const double* acc, long long i) {
    double s = acc ? acc[i] : 0.0;
    for (int j = 0; j < k; ++j) s = fma(a.w[j], (double)ld1(a.s[j] + i), s);
    return s;
}
template <bool V>
__global__ __launch_bounds__(256) void ema_combine_kernel(float* out, double* acc, long long n, int k, const CombineArgs a) {
    const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x, nth = (long long)gridDim.x * blockDim.x;
    if constexpr (V) {
        const long long n4 = n >> 2;
        for (long long i = tid; i < n4; i += nth) {
            double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
            if (acc) {
                const f64x2 lo = reinterpret_cast<const f64x2*>(acc)[2 * i], hi = reinterpret_cast<const f64x2*>(acc)[2 * i + 1];
                s0 = lo[0]; s1 = lo[1]; s2 = hi[0]; s3 = hi[1];
            }
#pragma unroll 4
            for (int j = 0; j < k; ++j) {
                const f32x4 x = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(a.s[j]) + i);
                const double w = a.w[j];
                s0 = fma(w, (double)x[0], s0); s1 = fma(w, (double)x[1], s1);
                s2 = fma(w, (double)x[2], s2); s3 = fma(w, (double)x[3], s3);
            }
            if (acc) {
                f64x2 lo, hi;
                lo[0] = s0; lo[1] = s1; hi[0] = s2; hi[1] = s3;
                reinterpret_cast<f64x2*>(acc)[2 * i] = lo; reinterpret_cast<f64x2*>(acc)[2 * i + 1] = hi;
            }
            if (out) {
                f32x4 o;
                o[0] = (float)s0; o[1] = (float)s1; o[2] = (float)s2; o[3] = (float)s3;
                __builtin_nontemporal_store(o, reinterpret_cast<f32x4*>(out) + i);
            }
        }
        if (tid < (n & 3)) {
            const long long i = (n4 << 2) + tid;
            const double s = combine_one(a, k, acc, i);
            if (acc) acc[i] = s;
            if (out) out[i] = (float)s;
        }
    } else {
        for (long long i = tid; i < n; i += nth) {
            const double s = combine_one(a, k, acc, i);
            if (acc) acc[i] = s;
            if (out) out[i] = (float)s;
        }
    }
}

// [a, a + na) and [b, b + nb) bytes share a byte
inline bool vd_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return a && b && x < y + nb && y < x + na;
}

constexpr int SUMSQ_BLOCKS = 1024;
}  // namespace

extern "C" size_t vd_sumsq_ws_bytes(int64_t) { return SUMSQ_BLOCKS * sizeof(float); }

extern "C" int vd_sumsq(const float* g, int64_t n, float* out1, float* ws, size_t ws_bytes, void* stream) {
    VD_REQUIRE(ws && ws_bytes >= SUMSQ_BLOCKS * sizeof(float), "vd_sumsq: workspace too small");
    VD_REQUIRE(vd_aligned16(g), "vd_sumsq: buffer must be 16-byte aligned");
    hipLaunchKernelGGL(sumsq_partial_kernel, dim3(SUMSQ_BLOCKS), dim3(256), 0, (hipStream_t)stream, g, (long long)n, ws);
    VD_LAUNCH_CHECK("sumsq_partial_kernel");
    hipLaunchKernelGGL(sumsq_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, ws, SUMSQ_BLOCKS, out1);
    VD_LAUNCH_CHECK("sumsq_final_kernel");
    return 0;
}

extern "C" int vd_adamw_ema(float* p, const float* g, float* m, float* v, float* ema, int64_t n, const float* gnorm_sq,
                            float max_norm, float lr, double beta1, double beta2, float eps, float wd, float bc1, float bc2,
                            double ema_decay, int64_t r_lo, int64_t r_hi, int32_t r_mode, float r_bc1, float r_bc2, void* stream) {
    VD_REQUIRE(r_mode >= 0 && r_mode <= 2, "vd_adamw_ema: r_mode must be 0, 1 or 2");
    VD_REQUIRE(r_mode == 0 || (0 <= r_lo && r_lo <= r_hi && r_hi <= n), "vd_adamw_ema: bad range [%lld, %lld)", (long long)r_lo, (long long)r_hi);
    VD_REQUIRE(r_mode != 2 || (r_bc1 > 0.f && r_bc2 > 0.f), "vd_adamw_ema: r_mode 2 needs positive bias corrections");
    long long grid = (n + 255) / 256;
    if (grid > 8192) grid = 8192;
    hipLaunchKernelGGL(adamw_ema_kernel, dim3((int)grid), dim3(256), 0, (hipStream_t)stream, p, g, m, v, ema, (long long)n,
                       gnorm_sq, max_norm, lr, (float)beta1, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), eps, wd, bc1, bc2,
                       (float)(1.0 - ema_decay), (long long)r_lo, (long long)r_hi, (int)r_mode,
                       r_mode == 2 ? r_bc1 : 1.f, r_mode == 2 ? r_bc2 : 1.f, (const float*)nullptr, (const int*)nullptr, 0.0, 0.0);
    VD_LAUNCH_CHECK("adamw_ema_kernel");
    return 0;
}

extern "C" int vd_adamw_ema_flagged(float* p, const float* g, float* m, float* v, float* ema, int64_t n, const float* gnorm_sq,
                                    float max_norm, float lr, double beta1, double beta2, float eps, float wd, float bc1, float bc2,
                                    double ema_decay, int64_t r_lo, int64_t r_hi, const float* r_flag, int32_t* r_steps,
                                    double r_beta1, double r_beta2, void* stream) {
    VD_REQUIRE(r_flag && r_steps, "vd_adamw_ema_flagged: needs the device flag and the device step counter");
    VD_REQUIRE(0 <= r_lo && r_lo <= r_hi && r_hi <= n, "vd_adamw_ema_flagged: bad range [%lld, %lld)", (long long)r_lo, (long long)r_hi);
    VD_REQUIRE(r_beta1 >= 0.0 && r_beta1 < 1.0 && r_beta2 >= 0.0 && r_beta2 < 1.0, "vd_adamw_ema_flagged: betas must lie in [0, 1)");
    long long grid = (n + 255) / 256;
    if (grid > 8192) grid = 8192;
    hipLaunchKernelGGL(adamw_ema_kernel, dim3((int)grid), dim3(256), 0, (hipStream_t)stream, p, g, m, v, ema, (long long)n,
                       gnorm_sq, max_norm, lr, (float)beta1, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), eps, wd, bc1, bc2,
                       (float)(1.0 - ema_decay), (long long)r_lo, (long long)r_hi, 3,
                       1.f, 1.f, r_flag, (const int*)r_steps, r_beta1, r_beta2);
    VD_LAUNCH_CHECK("adamw_ema_kernel");
    hipLaunchKernelGGL(cls_step_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, r_flag, (int*)r_steps);
    VD_LAUNCH_CHECK("cls_step_advance_kernel");
    return 0;
}

namespace {
template <int NP, typename... A>
void launch_emas(int grid, hipStream_t st, float* const* pema, const double* rate, A... a) {
    PemaArgs<NP> pe;
    for (int k = 0; k < NP; ++k) { pe.e[k] = pema[k]; pe.r[k] = (float)rate[k]; }
    hipLaunchKernelGGL(adamw_emas_kernel<NP>, dim3(grid), dim3(256), 0, st, a..., pe);
}
}  // namespace

extern "C" int vd_adamw_emas(float* p, const float* g, float* m, float* v, float* ema, int64_t n, const float* gnorm_sq, float max_norm,
                             float lr, double beta1, double beta2, float eps, float wd, float bc1, float bc2, double ema_decay,
                             int64_t r_lo, int64_t r_hi, int32_t r_mode, float r_bc1, float r_bc2,
                             const float* r_flag, int32_t* r_steps, double r_beta1, double r_beta2,
                             float* const* pema, const double* pema_rate, int32_t n_pema, void* stream) {
    VD_REQUIRE(p && g && m && v && n >= 0, "vd_adamw_emas: null buffer or negative n");
    VD_REQUIRE(n_pema >= 1 && n_pema <= PEMA_MAX, "vd_adamw_emas: 1..%d power shadows (got %d)", PEMA_MAX, (int)n_pema);
    VD_REQUIRE(pema && pema_rate, "vd_adamw_emas: needs the shadow pointers and their rates");
    if (r_flag) {
        VD_REQUIRE(r_steps, "vd_adamw_emas: the device flag needs the device step counter");
        VD_REQUIRE(0 <= r_lo && r_lo <= r_hi && r_hi <= n, "vd_adamw_emas: bad range [%lld, %lld)", (long long)r_lo, (long long)r_hi);
        VD_REQUIRE(r_beta1 >= 0.0 && r_beta1 < 1.0 && r_beta2 >= 0.0 && r_beta2 < 1.0, "vd_adamw_emas: betas must lie in [0, 1)");
    } else {
        VD_REQUIRE(r_mode >= 0 && r_mode <= 2, "vd_adamw_emas: r_mode must be 0, 1 or 2");
        VD_REQUIRE(r_mode == 0 || (0 <= r_lo && r_lo <= r_hi && r_hi <= n), "vd_adamw_emas: bad range [%lld, %lld)", (long long)r_lo, (long long)r_hi);
        VD_REQUIRE(r_mode != 2 || (r_bc1 > 0.f && r_bc2 > 0.f), "vd_adamw_emas: r_mode 2 needs positive bias corrections");
    }
    const size_t nb = (size_t)n * sizeof(float);
    const void* const others[5] = {p, g, m, v, ema};
    for (int k = 0; k < n_pema; ++k) {
        VD_REQUIRE(pema[k], "vd_adamw_emas: power shadow %d is null", k);
        VD_REQUIRE(pema_rate[k] > 0.0 && pema_rate[k] <= 1.0 && (float)pema_rate[k] > 0.f, "vd_adamw_emas: rate %d = %g outside (0, 1]", k, pema_rate[k]);
        for (int o = 0; o < 5; ++o)
            VD_REQUIRE(!vd_overlap(pema[k], nb, others[o], nb), "vd_adamw_emas: power shadow %d aliases p, g, m, v or ema", k);
        for (int o = 0; o < k; ++o)
            VD_REQUIRE(!vd_overlap(pema[k], nb, pema[o], nb), "vd_adamw_emas: power shadows %d and %d alias", o, k);
    }
    if (n == 0) return 0;
    long long grid = (n + 255) / 256;
    if (grid > 8192) grid = 8192;
    const hipStream_t st = (hipStream_t)stream;
    const bool fl = r_flag != nullptr;
#define VD_EMAS_LAUNCH(NP)                                                                                                               \
    launch_emas<NP>((int)grid, st, pema, pema_rate, p, g, m, v, ema, (long long)n, gnorm_sq, max_norm, lr, (float)beta1, (float)beta2,   \
                    (float)(1.0 - beta1), (float)(1.0 - beta2), eps, wd, bc1, bc2, (float)(1.0 - ema_decay), (long long)r_lo,            \
                    (long long)r_hi, fl ? 3 : (int)r_mode, !fl && r_mode == 2 ? r_bc1 : 1.f, !fl && r_mode == 2 ? r_bc2 : 1.f, r_flag,   \
                    (const int*)r_steps, fl ? r_beta1 : 0.0, fl ? r_beta2 : 0.0)
    switch (n_pema) {
        case 1: VD_EMAS_LAUNCH(1); break;
        case 2: VD_EMAS_LAUNCH(2); break;
        case 3: VD_EMAS_LAUNCH(3); break;
        default: VD_EMAS_LAUNCH(4); break;
    }
#undef VD_EMAS_LAUNCH
    VD_LAUNCH_CHECK("adamw_emas_kernel");
    if (fl) {
        hipLaunchKernelGGL(cls_step_advance_kernel, dim3(1), dim3(1), 0, st, r_flag, (int*)r_steps);
        VD_LAUNCH_CHECK("cls_step_advance_kernel");
    }
    return 0;
}

extern "C" int vd_ema_combine(float* out, double* acc, const float* const* src, const double* w, int32_t k, int64_t n, void* stream) {
    VD_REQUIRE(k >= 1 && k <= COMBINE_MAX, "vd_ema_combine: 1..%d sources (got %d)", COMBINE_MAX, (int)k);
    VD_REQUIRE(out || acc, "vd_ema_combine: needs out, acc or both");
    VD_REQUIRE(src && w && n >= 0, "vd_ema_combine: null source table / weights or negative n");
    VD_REQUIRE(!acc || (reinterpret_cast<uintptr_t>(acc) & 7) == 0, "vd_ema_combine: acc must be 8-byte aligned");
    CombineArgs a = {};
    int kk = 0;
    bool vec = vd_aligned16(out) && vd_aligned16(acc);
    for (int j = 0; j < k; ++j) {
        if (w[j] == 0.0) continue;                      // a source of weight 0 is not read
        VD_REQUIRE(src[j], "vd_ema_combine: source %d is null", j);
        VD_REQUIRE(!vd_overlap(src[j], (size_t)n * 4, out, (size_t)n * 4) && !vd_overlap(src[j], (size_t)n * 4, acc, (size_t)n * 8),
                   "vd_ema_combine: source %d aliases out or acc", j);
        vec = vec && vd_aligned16(src[j]);
        a.s[kk] = src[j]; a.w[kk] = w[j]; ++kk;
    }
    if (n == 0) return 0;
    if (vec && n >= 4) {
        long long grid = ((n >> 2) + 255) / 256;
        if (grid > 8192) grid = 8192;
        hipLaunchKernelGGL(ema_combine_kernel<true>, dim3((int)grid), dim3(256), 0, (hipStream_t)stream, out, acc, (long long)n, kk, a);
    } else {
        long long grid = (n + 255) / 256;
        if (grid > 8192) grid = 8192;
        hipLaunchKernelGGL(ema_combine_kernel<false>, dim3((int)grid), dim3(256), 0, (hipStream_t)stream, out, acc, (long long)n, kk, a);
    }
    VD_LAUNCH_CHECK("ema_combine_kernel");
    return 0;
}
