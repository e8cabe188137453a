// fid.hip -- fp64 feature statistics and matrix products of the Frechet Inception Distance (reference
// v_diffusion/metrics/fid_score.py).  One tile engine, C[i][j] (+)= sum_k A[k][i] B[k][j] with both operands row-major and K-major,
// fp64 accumulation on v_mfma_f64_16x16x4_f64, instantiated twice:
//
//   STATS  (vd_fid_accum): A = B = one batch of fp32 activations x[n][d]; the staged value is (double)x - shift[col], so with an
//          fp32-representable shift close to the data every difference and every product is exact and only the sums round.
//          outer[d][d] += the products, LOWER TRIANGLE OF 64 x 64 TILES ONLY (tile row >= tile column; the diagonal tiles in
//          full), sum[d] += the column sums (taken by the diagonal tiles from the operand they have staged anyway).
//   plain  (vd_atb_f64):   A[k][m], B[k][n] fp64, C[m][n] = A^T B.
//
// Structure: 4 waves own one 64 x 64 output tile (2 x 2 MFMA tiles of 16 x 16 per wave) and loop over ALL k rows in steps of 16:
// no split of the reduction, no atomics, one owner per output element -> the same call sequence gives bitwise identical results.
// The operands of the next step are loaded into registers while the current one is multiplied out of LDS (two LDS buffers, one
// barrier per step).  The MFMA's operand map is A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][j = lane & 15], one fp64 per lane:
// with K-major tiles in LDS a wave reads 16 consecutive doubles of 4 consecutive k rows, and the 80-double row pitch (640 B = 128 mod
// 256) puts the two rows of a 32-lane ds_read_b64 group on disjoint banks.  C/D map of the f64 shape: col = lane & 15,
// row = (lane >> 4) + 4 reg (NOT the f32 shapes' 4 (lane >> 4) + reg).
#include "common.h"

namespace {

typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int BT = 64;            // output tile edge
constexpr int BK = 16;            // k rows per step
constexpr int LDT = BT + 16;      // LDS row pitch in doubles
constexpr int TILE = BK * LDT;    // doubles per staged operand tile

struct AtbArgs {
    const void* A; const void* B; double* C;
    const double* shift; double* sum;      // STATS only
    long long k, lda, ldb, ldc;
    int m, n;
};

template <bool STATS> struct Raw;                                    // 4 consecutive columns of one k row, as loaded
template <> struct Raw<true> { f32x4 v; bool valid; };
template <> struct Raw<false> { f64x2 lo, hi; bool valid; };

template <bool STATS>
__device__ __forceinline__ void gload(Raw<STATS>& r, const void* base, long long ld, long long row, long long k, int col, bool in) {
    r.valid = in && row < k;
    if constexpr (STATS) {
        r.v = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        if (r.valid) r.v = *(const f32x4*)((const float*)base + row * ld + col);
    } else {
        r.lo = f64x2{0.0, 0.0}; r.hi = r.lo;
        if (r.valid) {
            const double* s = (const double*)base + row * ld + col;
            r.lo = *(const f64x2*)s; r.hi = *(const f64x2*)(s + 2);
        }
    }
}

// rows past k and columns past the matrix edge are staged as zeros: they add nothing to any sum
template <bool STATS>
__device__ __forceinline__ void lwrite(double* dst, const Raw<STATS>& r, const double* s) {
    f64x2 lo, hi;
    if constexpr (STATS) {
        lo = f64x2{(double)r.v[0] - s[0], (double)r.v[1] - s[1]};
        hi = f64x2{(double)r.v[2] - s[2], (double)r.v[3] - s[3]};
        if (!r.valid) { lo = f64x2{0.0, 0.0}; hi = lo; }
    } else {
        lo = r.lo; hi = r.hi;
    }
    *(f64x2*)dst = lo;
    *(f64x2*)(dst + 2) = hi;
}

template <bool STATS>
__global__ __launch_bounds__(256) void atb_f64_kernel(const AtbArgs p) {
    __shared__ __attribute__((aligned(16))) double smem[2 * 2 * TILE];
    const int ti = blockIdx.y, tj = blockIdx.x;
    if (STATS && tj > ti) return;                                    // lower triangle of tiles
    const bool diag = STATS && ti == tj;                             // B tile == A tile
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    const int i0 = ti * BT, j0 = tj * BT;

    // staging: thread -> k row tid / 16 of the step, columns 4 (tid % 16) .. + 3 of the tile (m, n are multiples of 16: all in or all out)
    const int sr = tid >> 4, sc = (tid & 15) * 4;
    const bool a_in = i0 + sc < p.m, b_in = !diag && j0 + sc < p.n;
    double sa[4] = {0.0, 0.0, 0.0, 0.0}, sb[4] = {0.0, 0.0, 0.0, 0.0};
    if constexpr (STATS) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (a_in) sa[q] = p.shift[i0 + sc + q];
            if (b_in) sb[q] = p.shift[j0 + sc + q];
        }
    }
    double* const wdst = smem + sr * LDT + sc;

    f64x4 acc[2][2];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int t = 0; t < 2; ++t) acc[s][t] = f64x4{0.0, 0.0, 0.0, 0.0};
    double csum = 0.0;                                               // diagonal tiles: column tid % 64, k rows 4 wave .. + 3 of each step

    const long long steps = (p.k + BK - 1) / BK;
    Raw<STATS> ra, rb;
    gload<STATS>(ra, p.A, p.lda, sr, p.k, i0 + sc, a_in);
    gload<STATS>(rb, p.B, p.ldb, sr, p.k, j0 + sc, b_in);
    for (long long c = 0; c < steps; ++c) {
        // (the buffer written here was last read two steps ago; every wave has passed the barrier of the step between)
        double* const As = smem + (c & 1) * 2 * TILE;
        double* const Bs = diag ? As : As + TILE;
        lwrite<STATS>(wdst + (c & 1) * 2 * TILE, ra, sa);
        if (!diag) lwrite<STATS>(wdst + (c & 1) * 2 * TILE + TILE, rb, sb);
        __syncthreads();
        if (c + 1 < steps) {
            gload<STATS>(ra, p.A, p.lda, (c + 1) * BK + sr, p.k, i0 + sc, a_in);
            gload<STATS>(rb, p.B, p.ldb, (c + 1) * BK + sr, p.k, j0 + sc, b_in);
        }
#pragma unroll
        for (int kk = 0; kk < BK / 4; ++kk) {
            const int off = (kk * 4 + (lane >> 4)) * LDT + (lane & 15);
            double a[2], b[2];
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                a[s] = As[off + wm * 32 + s * 16];
                b[s] = Bs[off + wn * 32 + s * 16];
            }
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int t = 0; t < 2; ++t) acc[s][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s], b[t], acc[s][t], 0, 0, 0);
        }
        if (diag) {
#pragma unroll
            for (int q = 0; q < 4; ++q) csum += As[(wave * 4 + q) * LDT + lane];
        }
    }

    // epilogue: register r of lane l is C[row (l >> 4) + 4 r][col l & 15] of its 16 x 16 tile
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int ib = i0 + wm * 32 + s * 16;
        if (ib >= p.m) continue;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int jb = j0 + wn * 32 + t * 16;
            if (jb >= p.n) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                double* o = p.C + (long long)(ib + (lane >> 4) + 4 * r) * p.ldc + jb + (lane & 15);
                if constexpr (STATS) *o += acc[s][t][r];
                else *o = acc[s][t][r];
            }
        }
    }

    if (diag) {
        // column sums: the four waves' partial sums in wave order
        __syncthreads();
        smem[wave * BT + lane] = csum;
        __syncthreads();
        if (tid < BT && i0 + tid < p.m) p.sum[i0 + tid] += ((smem[tid] + smem[BT + tid]) + smem[2 * BT + tid]) + smem[3 * BT + tid];
    }
}

// shift[c] = the fp32-rounded mean of column c (rows summed in order, fp64)
__global__ __launch_bounds__(256) void fid_shift_kernel(const float* __restrict__ x, long long n, int d, long long ldx,
                                                        double* __restrict__ shift) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= d) return;
    double s = 0.0;
    for (long long i = 0; i < n; ++i) s += (double)x[i * ldx + c];
    shift[c] = (double)(float)(s / (double)n);
}

bool stats_domain(const char* who, const float* x, int64_t n, int32_t d, int64_t ldx) {
    if (!(n >= 1 && d >= 16 && d % 16 == 0 && ldx >= d && ldx % 4 == 0)) {
        vd_set_error("%s: n = %lld, d = %d, ldx = %lld (need n >= 1, d a positive multiple of 16, ldx >= d and a multiple of 4)", who,
                     (long long)n, d, (long long)ldx);
        return false;
    }
    if (!vd_aligned16(x)) { vd_set_error("%s: x must be 16-byte aligned", who); return false; }
    return true;
}

}  // namespace

extern "C" int vd_fid_shift(const float* x, int64_t n, int32_t d, int64_t ldx, double* shift, void* stream) {
    if (!stats_domain("vd_fid_shift", x, n, d, ldx)) return 1;
    hipLaunchKernelGGL(fid_shift_kernel, dim3((unsigned)((d + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, (long long)n, d,
                       (long long)ldx, shift);
    VD_LAUNCH_CHECK("fid_shift_kernel");
    return 0;
}

extern "C" int vd_fid_accum(const float* x, int64_t n, int32_t d, int64_t ldx, const double* shift, double* sum, double* outer,
                            void* stream) {
    if (!stats_domain("vd_fid_accum", x, n, d, ldx)) return 1;
    VD_REQUIRE(vd_aligned16(shift) && vd_aligned16(sum) && vd_aligned16(outer), "vd_fid_accum: shift, sum and outer must be 16-byte aligned");
    AtbArgs a{};
    a.A = x; a.B = x; a.C = outer; a.shift = shift; a.sum = sum;
    a.k = n; a.lda = ldx; a.ldb = ldx; a.ldc = d; a.m = d; a.n = d;
    const unsigned t = (unsigned)((d + BT - 1) / BT);
    hipLaunchKernelGGL(atb_f64_kernel<true>, dim3(t, t), dim3(256), 0, (hipStream_t)stream, a);
    VD_LAUNCH_CHECK("atb_f64_kernel<stats>");
    return 0;
}

extern "C" int vd_atb_f64(const double* A, const double* B, double* C, int64_t k, int32_t m, int32_t n, int64_t lda, int64_t ldb,
                          int64_t ldc, void* stream) {
    VD_REQUIRE(k >= 1 && m >= 16 && m % 16 == 0 && n >= 16 && n % 16 == 0, "vd_atb_f64: k = %lld, m = %d, n = %d (need k >= 1, m and n "
               "positive multiples of 16)", (long long)k, m, n);
    VD_REQUIRE(lda >= m && ldb >= n && ldc >= n && lda % 2 == 0 && ldb % 2 == 0, "vd_atb_f64: lda = %lld, ldb = %lld, ldc = %lld (need "
               "lda >= m, ldb >= n, ldc >= n, lda and ldb even)", (long long)lda, (long long)ldb, (long long)ldc);
    VD_REQUIRE(vd_aligned16(A) && vd_aligned16(B) && vd_aligned16(C), "vd_atb_f64: A, B and C must be 16-byte aligned");
    AtbArgs a{};
    a.A = A; a.B = B; a.C = C;
    a.k = k; a.lda = lda; a.ldb = ldb; a.ldc = ldc; a.m = m; a.n = n;
    hipLaunchKernelGGL(atb_f64_kernel<false>, dim3((unsigned)((n + BT - 1) / BT), (unsigned)((m + BT - 1) / BT)), dim3(256), 0,
                       (hipStream_t)stream, a);
    VD_LAUNCH_CHECK("atb_f64_kernel");
    return 0;
}
