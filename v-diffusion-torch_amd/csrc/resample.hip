// resample.hip -- loss-aware timestep resampling (Nichol & Dhariwal 2021, section 3.3: t ~ sqrt(E[L_t^2]), loss reweighted by
// 1/(T p_t)) with the loss history resident on the device: one launch draws a batch of timesteps, one launch writes a batch of
// (timestep, loss) rows into the per-timestep ring.  No counterpart in the reference (improved-diffusion keeps the history in numpy
// and draws on the host).  Both kernels are latency bound: a (T, K) fp32 table of 40 KB at T = 1000, K = 10.
#include "common.h"

#include <cmath>

namespace {

enum { LSM_THREADS = 1024, LSM_WAVES = LSM_THREADS / 64, LSM_LDS_T = 4096 };
enum { UPD_THREADS = 256, UPD_TILE = 1024 };

// m_t = sqrt(sum_k h[t][k]^2 / K) in fp64, k ascending (the square of an fp32 is exact in fp64: fma and multiply-add give the same bits)
__device__ __forceinline__ double lsm_rms(const float* row, int K) {
    double acc = 0.0;
    for (int k = 0; k < K; ++k) {
        const double h = (double)row[k];
        acc = fma(h, h, acc);
    }
    return sqrt(acc / (double)K);
}

// q_t: one expression for the scan and for the weight of a drawn index, so that both see the same bits
__device__ __forceinline__ double lsm_prob(double m, double S, bool flat, double eps, double Td) {
    return flat ? 1.0 / Td : (1.0 - eps) * m / S + eps / Td;
}

// inclusive scan of one value per thread over the workgroup, fixed order: Hillis-Steele over the 64 lanes of a wave, then the totals of
// the waves in front added in wave order.  sh: LSM_WAVES doubles.  The last thread's value is the total.
__device__ __forceinline__ double lsm_block_scan(double v, double* sh) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double up = __shfl_up(v, o, 64);
        if (lane >= o) v += up;
    }
    if (lane == 63) sh[w] = v;
    __syncthreads();
    double off = 0.0;
    for (int i = 0; i < w; ++i) off += sh[i];
    __syncthreads();
    return off + v;
}

// sum over the workgroup, fixed order: butterfly over the lanes, wave totals in wave order; every thread receives the same bits
__device__ __forceinline__ double lsm_block_sum(double v, double* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
    for (int i = 0; i < LSM_WAVES; ++i) t += sh[i];
    __syncthreads();
    return t;
}

// #{i : c[i] <= u} of a non-decreasing c[0..T): binary search, at most 17 probes for T = 65536
__device__ __forceinline__ int lsm_upper_bound(const double* c, int T, double u) {
    int lo = 0, hi = T;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (c[mid] <= u) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// ONE workgroup does the whole draw and waits on no other:
//   1. warmed up?  every count[t] == K                                                  (__syncthreads_and over all t)
//   2. m_t for t = c*1024 + thread, chunk after chunk, left in cdf[t]; S = sum of the threads' partial sums in fixed order
//   3. q_t from m_t, inclusive scan chunk after chunk with the running total carried in a register every thread holds; cdf[t]
//      written (and kept in LDS when T <= LSM_LDS_T)
//   4. thread b, b + 1024, ...: binary search of u[b], q of the index found recomputed from its history row, weight, t
// A thread re-reads in 3 only what it wrote itself in 2; the searches of 4 follow a workgroup barrier behind a device-scope fence.
__global__ __launch_bounds__(LSM_THREADS) void lsm_draw_kernel(const float* hist, const int* count, const double* u, double* cdf,
                                                               double* t_out, int* idx_out, float* w_out, int T, int K, int B, double eps) {
    __shared__ double sh[LSM_WAVES];
    __shared__ double scdf[LSM_LDS_T];
    const int tid = threadIdx.x;
    const double Td = (double)T;
    int full = 1;
    for (int t = tid; t < T; t += LSM_THREADS) full &= (count[t] == K) ? 1 : 0;
    const bool warm = __syncthreads_and(full) != 0;
    if (!warm) {
        // the draw of HotPathTrainer's uniform grid, from a double: idx = floor(u T), weight exactly one; cdf = the uniform one
        for (int t = tid; t < T; t += LSM_THREADS) cdf[t] = (double)(t + 1) / Td;
        for (int b = tid; b < B; b += LSM_THREADS) {
            const double x = u[b] * Td;
            int idx = x >= 1.0 ? (x < Td ? (int)floor(x) : T - 1) : 0;            // (a NaN or a negative u lands on 0)
            idx = idx > T - 1 ? T - 1 : idx;
            idx_out[b] = idx;
            w_out[b] = 1.0f;
            t_out[b] = (double)(idx + 1) / Td;
        }
        return;
    }
    double part = 0.0;
    for (int t = tid; t < T; t += LSM_THREADS) {
        const double m = lsm_rms(hist + (long long)t * K, K);
        cdf[t] = m;
        part += m;
    }
    const double S = lsm_block_sum(part, sh);
    const bool flat = !(S > 0.0) || !(S <= 1.7976931348623157e308);              // zero, NaN or Inf: the uniform distribution
    const bool in_lds = T <= LSM_LDS_T;
    double carry = 0.0;
    for (int base = 0; base < T; base += LSM_THREADS) {                          // (uniform trip count: every thread meets every barrier)
        const int t = base + tid;
        const double q = t < T ? lsm_prob(cdf[t], S, flat, eps, Td) : 0.0;
        const double c = carry + lsm_block_scan(q, sh);
        if (t < T) {
            cdf[t] = c;
            if (in_lds) scdf[t] = c;
        }
        if (tid == LSM_THREADS - 1) sh[0] = c;
        __syncthreads();
        carry = sh[0];
        __syncthreads();
    }
    __threadfence();
    __syncthreads();
    const double* table = in_lds ? scdf : cdf;
    for (int b = tid; b < B; b += LSM_THREADS) {
        int idx = lsm_upper_bound(table, T, u[b]);
        idx = idx > T - 1 ? T - 1 : idx;
        const double q = lsm_prob(lsm_rms(hist + (long long)idx * K, K), S, flat, eps, Td);
        idx_out[b] = idx;
        w_out[b] = (float)(1.0 / (Td * q));
        t_out[b] = (double)(idx + 1) / Td;
    }
}

// one thread per timestep walks the n rows in row order, UPD_TILE rows at a time through LDS (a row that is skipped -- index outside
// [0, T), loss not finite -- is staged as index -1 and matches no thread); a match writes the loss into the thread's ring slot and
// advances its position and count, which live in registers until the end.  Writes of one thread to one address keep program order:
// the state equals the sequential loop's, also when a timestep occurs many times in one call.
__global__ __launch_bounds__(UPD_THREADS) void lsm_update_kernel(float* hist, int* count, int* pos, const int* idx, const float* loss, int n,
                                                                 int T, int K) {
    __shared__ __attribute__((aligned(16))) int sidx[UPD_TILE];
    __shared__ float sloss[UPD_TILE];
    const int t = blockIdx.x * UPD_THREADS + threadIdx.x;
    const bool mine = t < T;
    int p = 0, c = 0;
    if (mine) {
        p = pos[t];
        c = count[t];
        if ((unsigned)p >= (unsigned)K) p = 0;                                    // (a position outside the ring can come from a foreign checkpoint only)
    }
    float* ring = hist + (long long)(mine ? t : 0) * K;
    for (int base = 0; base < n; base += UPD_TILE) {
        const int rows = n - base < UPD_TILE ? n - base : UPD_TILE;
        for (int r = threadIdx.x; r < UPD_TILE; r += UPD_THREADS) {
            int i = -1;
            float l = 0.f;
            if (r < rows) {
                i = idx[base + r];
                l = loss[base + r];
                if (i < 0 || i >= T || !(fabsf(l) <= 3.402823466e+38f)) i = -1;
            }
            sidx[r] = i;
            sloss[r] = l;
        }
        __syncthreads();
        if (mine) {
            const int4* s4 = reinterpret_cast<const int4*>(sidx);
            const int quads = (rows + 3) >> 2;                                    // (everything staged behind the last row holds -1)
            for (int j = 0; j < quads; j += 4) {                                  // 16 rows per trip: four LDS reads in flight
                const int4 v0 = s4[j], v1 = s4[j + 1], v2 = s4[j + 2], v3 = s4[j + 3];
                const int e[16] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w, v2.x, v2.y, v2.z, v2.w, v3.x, v3.y, v3.z, v3.w};
                bool hit = false;
#pragma unroll
                for (int k = 0; k < 16; ++k) hit |= e[k] == t;
                if (hit) {
#pragma unroll
                    for (int k = 0; k < 16; ++k) {
                        if (e[k] == t) {
                            ring[p] = sloss[4 * j + k];
                            p = p + 1 == K ? 0 : p + 1;
                            c = c < K ? c + 1 : K;
                        }
                    }
                }
            }
        }
        __syncthreads();
    }
    if (mine && n > 0) {
        pos[t] = p;
        count[t] = c;
    }
}

}  // namespace

extern "C" int vd_lsm_draw(const float* hist, const int32_t* count, const double* u, double* cdf, double* t_out, int32_t* idx_out,
                           float* w_out, int32_t T, int32_t K, int32_t B, double uniform_prob, void* stream) {
    VD_REQUIRE(hist && count && u && cdf && t_out && idx_out && w_out, "vd_lsm_draw: null pointer");
    VD_REQUIRE(T >= 1 && T <= 65536, "vd_lsm_draw: 1 <= T <= 65536 (T=%d)", T);
    VD_REQUIRE(K >= 1, "vd_lsm_draw: K >= 1 (K=%d)", K);
    VD_REQUIRE(B >= 1, "vd_lsm_draw: empty batch (B=%d)", B);
    VD_REQUIRE(uniform_prob >= 0.0 && uniform_prob <= 1.0, "vd_lsm_draw: uniform_prob in [0, 1], got %g", uniform_prob);
    hipLaunchKernelGGL(lsm_draw_kernel, dim3(1), dim3(LSM_THREADS), 0, (hipStream_t)stream, hist, count, u, cdf, t_out, idx_out, w_out,
                       (int)T, (int)K, (int)B, uniform_prob);
    VD_LAUNCH_CHECK("lsm_draw_kernel");
    return 0;
}

extern "C" int vd_lsm_update(float* hist, int32_t* count, int32_t* pos, const int32_t* idx, const float* loss, int32_t n, int32_t T,
                             int32_t K, void* stream) {
    VD_REQUIRE(T >= 1 && T <= 65536, "vd_lsm_update: 1 <= T <= 65536 (T=%d)", T);
    VD_REQUIRE(K >= 1, "vd_lsm_update: K >= 1 (K=%d)", K);
    VD_REQUIRE(n >= 0, "vd_lsm_update: negative row count (n=%d)", n);
    if (n == 0) return 0;
    VD_REQUIRE(hist && count && pos && idx && loss, "vd_lsm_update: null pointer");
    hipLaunchKernelGGL(lsm_update_kernel, dim3((T + UPD_THREADS - 1) / UPD_THREADS), dim3(UPD_THREADS), 0, (hipStream_t)stream, hist, count,
                       pos, idx, loss, (int)n, (int)T, (int)K);
    VD_LAUNCH_CHECK("lsm_update_kernel");
    return 0;
}
