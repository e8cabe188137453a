// metrics.hip -- fused k-NN passes of the improved precision / recall metric (Kynkaanniemi et al. 2019; reference
// v_diffusion/metrics/precision_recall.py).  Every pass is an all-pairs distance computation between two sets of fp16 feature
// rows (eval.py: 50 000 x 4 096) reduced per row as it is produced; the distance matrix never exists in memory.
//
//   d2(x, y) = max(|x|^2 + |y|^2 - 2 x.y, 0) in fp32, dist = sqrtf(d2) (correctly rounded)
//   knn_kth:  out[i] = kth-th smallest dist(q_i, c_j) over j, with multiplicity (torch.kthvalue(kth) of a distance row)
//   hits:     hit[i] = 1 iff some j has dist(q_i, s_j) <= radius[j]
//
// Tile engine: 4 waves, 128 query rows x 128 candidate rows per tile, K step 64 fp16, both operands staged into LDS by
// global_load_lds (16 B per lane, double buffered).  v_mfma_f32_32x32x16_f16 with the CANDIDATE rows as operand A and the QUERY
// rows as operand B puts one query on each lane (column = lane & 31) and 16 candidates in its 16 accumulator registers (rows
// (r & 3) + 8 (r >> 2) + 4 (lane >> 5)): the per-query reduction is lane-local.  The k-th pass keeps a sorted list of the L
// smallest d2 per lane (insertion a[i+1] = med3(a[i], v, a[i+1]) from the top down, then a[0] = min(a[0], v): L VALU per
// candidate, order-independent and exact); the hit pass compares d2 against a per-candidate d2 threshold equivalent to
// sqrtf(d2) <= radius.  Lanes l / l + 32 and the two waves that share query rows are merged at the end of the workgroup.
//
// The candidate range is split over S workgroups per query tile (S from the shapes only, so the workspace size is a pure
// function of them); the k-th pass writes S partial lists [S][nq][L] and a small kernel merges them in a fixed order.  The hit
// pass stores hit[i] = 1 from whichever workgroup finds one (all writers store the same byte; no atomics).
//
// Self-distance: the squared norms come from the same MFMA chain (same instruction, same k order, accumulator from 0) as the
// tile engine's dot products, so for identical rows x.y == |x|^2 == |y|^2 bitwise and d2 is exactly 0.
#include "common.h"

namespace {

typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

constexpr int BM = 128, BN = 128, BK = 64;      // query rows, candidate rows, fp16 per K step
constexpr int TILE_BYTES = BM * BK * 2;         // 16 KiB per operand tile
constexpr float INF = __builtin_inff();

struct KnnArgs {
    const uint16_t* q; const float* q_sq; long long nq;
    const uint16_t* c; const float* c_sq; long long nc;
    const float* thr;                           // hit pass: per-candidate d2 threshold
    int d, splits, nct;                         // feature length (multiple of BK), column splits, candidate tiles
    float* part;                                // k-th pass: [splits][nq][L]
    uint8_t* hit;                               // hit pass: [nq]
};

// LDS image of a 128-row x 64-fp16 tile: 128-B rows, 16-B chunk c of row r stored in slot c ^ ((r >> 1) & 7) -- ds_read_b128 of one
// chunk over 16 consecutive rows touches 16 distinct 16-B positions of the 256-B bank row.
__device__ __forceinline__ int lds_off(int r, int c) { return r * 128 + ((c ^ ((r >> 1) & 7)) << 4); }

__device__ __forceinline__ void list_insert(float* a, int L, float v) {
    for (int i = L - 2; i >= 0; --i) a[i + 1] = __builtin_amdgcn_fmed3f(a[i], v, a[i + 1]);
    a[0] = fminf(a[0], v);
}

__device__ __forceinline__ float d2_of(float dot, float nq, float nc) { return fmaxf(fmaf(-2.0f, dot, nq + nc), 0.0f); }

template <int L, bool HITS>
__global__ __launch_bounds__(256, 2) void knn_tile_kernel(const KnnArgs p) {
    __shared__ __attribute__((aligned(1024))) unsigned char smem[2 * 2 * TILE_BYTES];
    constexpr int LL = HITS ? 1 : L;
    const int tid = threadIdx.x, lane = tid & 63, li = lane & 31, lh = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wq = wave >> 1, wc = wave & 1;     // query half / candidate half of the tile owned by this wave

    // XCD-aware order (gemm.hip's remap): workgroups are dealt round-robin over the 8 XCDs; give every XCD a contiguous run of
    // (query tile, split) pairs, query tile fastest, so the workgroups of one L2 stream the same candidate panels.  Bijective.
    const unsigned T = gridDim.x * gridDim.y, lin = blockIdx.y * gridDim.x + blockIdx.x;
    unsigned t = lin;
    if (T >= 16) {
        const unsigned qq = T / 8, r = T % 8, xcd = lin % 8, slot = lin / 8;
        t = (xcd < r ? xcd * (qq + 1) : r * (qq + 1) + (xcd - r) * qq) + slot;
    }
    const int qt = (int)(t % gridDim.x), split = (int)(t / gridDim.x);
    const long long m0 = (long long)qt * BM;
    const int ct0 = (int)((long long)split * p.nct / p.splits), ct1 = (int)((long long)(split + 1) * p.nct / p.splits);
    const int KT = p.d / BK;

    // staging: 16 wave-instructions of 1 KiB (8 rows) per operand tile, 4 per wave; lane -> row g*8 + lane/8, LDS slot lane%8,
    // global chunk slot ^ swizzle (the swizzle sits on the source address: the LDS side of global_load_lds is lane-linear)
    const int srow = lane >> 3;
    const uint16_t* qsrc[4];
    int crow[4], cchunk[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int r = (j * 4 + wave) * 8 + srow;
        const int ch = (lane & 7) ^ ((r >> 1) & 7);
        const long long qi = m0 + r < p.nq ? m0 + r : p.nq - 1;          // tail rows re-read the last row; their results are masked
        qsrc[j] = p.q + qi * p.d + ch * 8;
        crow[j] = r; cchunk[j] = ch;
    }
    const uint16_t* csrc[4];
    auto set_ctile = [&](int ct) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long ci = (long long)ct * BN + crow[j];
            csrc[j] = p.c + (ci < p.nc ? ci : p.nc - 1) * p.d + cchunk[j] * 8;
        }
    };
    auto issue = [&](int buf, int kt) {
        unsigned char* qs = smem + buf * 2 * TILE_BYTES;
        unsigned char* cs = qs + TILE_BYTES;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            __builtin_amdgcn_global_load_lds((const void*)(qsrc[j] + kt * BK), (lds_ptr_t)(qs + (j * 4 + wave) * 1024), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((const void*)(csrc[j] + kt * BK), (lds_ptr_t)(cs + (j * 4 + wave) * 1024), 16, 0, 0);
        }
    };

    // per-lane query norms (queries wq*64 + qs*32 + li)
    float qn[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const long long qi = m0 + wq * 64 + s * 32 + li;
        qn[s] = p.q_sq[qi < p.nq ? qi : p.nq - 1];
    }
    float list[2][LL];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int i = 0; i < LL; ++i) list[s][i] = INF;
    bool hit[2] = {false, false};

    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = f32x16{};

    int ct = ct0, kt = 0, buf = 0;
    set_ctile(ct);
    issue(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    while (ct < ct1) {
        // next step's operands into the other buffer (its last readers passed the barrier that ended the previous step)
        int nkt = kt + 1, nct = ct;
        if (nkt == KT) { nkt = 0; ++nct; }
        if (nct < ct1) {
            if (nct != ct) set_ctile(nct);
            issue(buf ^ 1, nkt);
        }
        const unsigned char* qs = smem + buf * 2 * TILE_BYTES;
        const unsigned char* cs = qs + TILE_BYTES;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const int ch = kk * 2 + lh;
            f16x8 fa[2], fb[2];
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                fa[s] = *(const f16x8*)(cs + lds_off(wc * 64 + s * 32 + li, ch));
                fb[s] = *(const f16x8*)(qs + lds_off(wq * 64 + s * 32 + li, ch));
            }
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[a], fb[b], acc[a][b], 0, 0, 0);
        }
        if (kt == KT - 1) {
            // epilogue of candidate tile ct: candidate row of register r = (r & 3) + 8 (r >> 2) + 4 lh within the 32-row sub-tile
            const long long n0 = (long long)ct * BN + wc * 64;
            const bool tail = (long long)ct * BN + BN > p.nc;
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                float cn[16], tv[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const long long j = n0 + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                    const long long jc = j < p.nc ? j : p.nc - 1;
                    cn[r] = p.c_sq[jc];
                    tv[r] = HITS ? p.thr[jc] : 0.0f;
                    if (tail && j >= p.nc) { cn[r] = INF; tv[r] = -1.0f; }   // masked candidates: d2 = +inf, never listed, never a hit
                }
#pragma unroll
                for (int b = 0; b < 2; ++b) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float v = d2_of(acc[a][b][r], qn[b], cn[r]);
                        if constexpr (HITS) hit[b] |= v <= tv[r];
                        else list_insert(list[b], L, v);
                    }
                    acc[a][b] = f32x16{};
                }
            }
            ++ct;
        }
        kt = nkt;
        buf ^= 1;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }

    // ---- merge: lanes l / l + 32 (same query, other candidates), then the two waves of a query half through LDS
    if constexpr (HITS) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const long long qi = m0 + wq * 64 + s * 32 + li;
            const int other = __shfl_xor((int)hit[s], 32);            // every lane takes part in the exchange
            const bool h = hit[s] || other != 0;
            if (h && lh == 0 && qi < p.nq) p.hit[qi] = 1;
        }
    } else {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            float other[L];
#pragma unroll
            for (int i = 0; i < L; ++i) other[i] = __shfl_xor(list[s][i], 32);
#pragma unroll
            for (int i = 0; i < L; ++i) list_insert(list[s], L, other[i]);
        }
        float* xl = (float*)smem;                                  // [wq][s][i][li]; the staging buffers are idle now
        if (wc == 1 && lh == 0) {
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int i = 0; i < L; ++i) xl[((wq * 2 + s) * L + i) * 32 + li] = list[s][i];
        }
        __syncthreads();
        if (wc == 0 && lh == 0) {
#pragma unroll
            for (int s = 0; s < 2; ++s) {
#pragma unroll
                for (int i = 0; i < L; ++i) list_insert(list[s], L, xl[((wq * 2 + s) * L + i) * 32 + li]);
                const long long qi = m0 + wq * 64 + s * 32 + li;
                if (qi < p.nq) {
                    float* o = p.part + ((long long)split * p.nq + qi) * L;
#pragma unroll
                    for (int i = 0; i < L; i += 4) *(f32x4*)(o + i) = f32x4{list[s][i], list[s][i + 1], list[s][i + 2], list[s][i + 3]};
                }
            }
        }
    }
}

// out[i] = sqrtf(kth-th smallest of the `splits` partial lists of row i), merged in split order
template <int L>
__global__ __launch_bounds__(256) void knn_finish_kernel(const float* __restrict__ part, long long nq, int splits, int kth,
                                                         float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= nq) return;
    float a[L];
#pragma unroll
    for (int k = 0; k < L; ++k) a[k] = part[i * L + k];
    for (int s = 1; s < splits; ++s) {
        const float* o = part + ((long long)s * nq + i) * L;
#pragma unroll
        for (int k = 0; k < L; ++k) list_insert(a, L, o[k]);
    }
    float v = a[0];
#pragma unroll
    for (int k = 1; k < L; ++k) v = (k == kth - 1) ? a[k] : v;
    out[i] = sqrtf(v);
}

// squared row norms through the tile engine's MFMA chain (see the file comment): one wave per 32 rows, operand A = operand B = the
// rows' own fragments, the diagonal of the 32 x 32 product read out of the accumulator
__global__ __launch_bounds__(256) void rows_sqnorm_kernel(const uint16_t* __restrict__ x, long long n, int d, float* __restrict__ sq) {
    const int lane = threadIdx.x & 63, li = lane & 31, lh = lane >> 5;
    const long long r0 = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 32;
    if (r0 >= n) return;
    const long long ri = r0 + li < n ? r0 + li : n - 1;
    const uint16_t* src = x + ri * d + lh * 8;
    f32x16 acc = f32x16{};
    for (int k = 0; k < d; k += 16) {
        const f16x8 f = *(const f16x8*)(src + k);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(f, f, acc, 0, 0, 0);
    }
    // element (li, li) sits in the lane of half (li >> 2) & 1, register (li & 3) + 4 (li >> 3)
    float v = 0.0f;
#pragma unroll
    for (int r = 0; r < 16; ++r) v = (r == (li & 3) + 4 * (li >> 3)) ? acc[r] : v;
    if (lh == ((li >> 2) & 1) && r0 + li < n) sq[r0 + li] = v;
}

// largest fp32 t with sqrtf(t) <= radius (sqrtf is monotone, so d2 <= t  <=>  sqrtf(d2) <= radius); NaN / negative radius: -1 (no hit)
__global__ __launch_bounds__(256) void radius_threshold_kernel(const float* __restrict__ radius, long long n, float* __restrict__ thr) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float r = radius[i];
    float t;
    if (!(r >= 0.0f)) t = -1.0f;
    else if (r == INF) t = INF;
    else {
        t = r * r;
        // (t >= 0: the neighbouring floats are the bit patterns -1 / +1)
        while (t > 0.0f && sqrtf(t) > r) t = __uint_as_float(__float_as_uint(t) - 1u);
        while (t < INF && sqrtf(__uint_as_float(__float_as_uint(t) + 1u)) <= r) t = __uint_as_float(__float_as_uint(t) + 1u);
    }
    thr[i] = t;
}

int splits_for(long long nq, long long nc) {
    const long long nqt = (nq + BM - 1) / BM, nct = (nc + BN - 1) / BN;
    long long s = (4096 + nqt - 1) / nqt;                 // ~4096 workgroups: the tail round is a small share of the pass
    const long long smax = nct / 4 > 1 ? nct / 4 : 1;     // >= 4 candidate tiles per workgroup
    if (s > smax) s = smax;
    return (int)(s < 1 ? 1 : s);
}

int list_len(int kth) { return kth <= 4 ? 4 : kth <= 8 ? 8 : 16; }

unsigned blocks_for(long long n) { return (unsigned)((n + 255) / 256); }

}  // namespace

extern "C" int vd_rows_sqnorm_f16(const uint16_t* x, int64_t n, int32_t d, float* sq, void* stream) {
    VD_REQUIRE(n >= 1 && d >= BK && d % BK == 0, "vd_rows_sqnorm_f16: n = %lld, d = %d (need n >= 1, d a positive multiple of %d)",
               (long long)n, d, BK);
    VD_REQUIRE(vd_aligned16(x), "vd_rows_sqnorm_f16: x must be 16-byte aligned");
    hipLaunchKernelGGL(rows_sqnorm_kernel, dim3((unsigned)((n + 127) / 128)), dim3(256), 0, (hipStream_t)stream, x, (long long)n, d, sq);
    VD_LAUNCH_CHECK("rows_sqnorm_kernel");
    return 0;
}

extern "C" size_t vd_knn_kth_ws_bytes(int64_t nq, int64_t nc, int32_t kth) {
    if (nq < 1 || nc < 1 || kth < 1 || kth > 16) return 0;
    return (size_t)splits_for(nq, nc) * (size_t)nq * (size_t)list_len(kth) * sizeof(float);
}

extern "C" int vd_knn_kth_f16(const uint16_t* q, const float* q_sq, int64_t nq, const uint16_t* c, const float* c_sq, int64_t nc,
                              int32_t d, int32_t kth, float* out, void* ws, size_t ws_bytes, void* stream) {
    VD_REQUIRE(nq >= 1 && nc >= 1, "vd_knn_kth_f16: empty set (nq = %lld, nc = %lld)", (long long)nq, (long long)nc);
    VD_REQUIRE(kth >= 1 && kth <= 16 && kth <= nc, "vd_knn_kth_f16: kth = %d outside [1, min(16, nc = %lld)]", kth, (long long)nc);
    VD_REQUIRE(d >= BK && d % BK == 0, "vd_knn_kth_f16: d = %d is not a positive multiple of %d (pad with zeros)", d, BK);
    VD_REQUIRE(vd_aligned16(q) && vd_aligned16(c) && vd_aligned16(ws), "vd_knn_kth_f16: q, c and ws must be 16-byte aligned");
    VD_REQUIRE(ws_bytes >= vd_knn_kth_ws_bytes(nq, nc, kth), "vd_knn_kth_f16: ws_bytes %zu < vd_knn_kth_ws_bytes %zu", ws_bytes,
               vd_knn_kth_ws_bytes(nq, nc, kth));
    KnnArgs a{};
    a.q = q; a.q_sq = q_sq; a.nq = nq; a.c = c; a.c_sq = c_sq; a.nc = nc; a.d = d;
    a.splits = splits_for(nq, nc); a.nct = (int)((nc + BN - 1) / BN); a.part = (float*)ws;
    const dim3 grid((unsigned)((nq + BM - 1) / BM), (unsigned)a.splits), blk(256);
    hipStream_t st = (hipStream_t)stream;
    const int L = list_len(kth);
    if (L == 4) {
        hipLaunchKernelGGL((knn_tile_kernel<4, false>), grid, blk, 0, st, a);
        VD_LAUNCH_CHECK("knn_tile_kernel<4>");
        hipLaunchKernelGGL(knn_finish_kernel<4>, dim3(blocks_for(nq)), dim3(256), 0, st, a.part, (long long)nq, a.splits, kth, out);
    } else if (L == 8) {
        hipLaunchKernelGGL((knn_tile_kernel<8, false>), grid, blk, 0, st, a);
        VD_LAUNCH_CHECK("knn_tile_kernel<8>");
        hipLaunchKernelGGL(knn_finish_kernel<8>, dim3(blocks_for(nq)), dim3(256), 0, st, a.part, (long long)nq, a.splits, kth, out);
    } else {
        hipLaunchKernelGGL((knn_tile_kernel<16, false>), grid, blk, 0, st, a);
        VD_LAUNCH_CHECK("knn_tile_kernel<16>");
        hipLaunchKernelGGL(knn_finish_kernel<16>, dim3(blocks_for(nq)), dim3(256), 0, st, a.part, (long long)nq, a.splits, kth, out);
    }
    VD_LAUNCH_CHECK("knn_finish_kernel");
    return 0;
}

extern "C" size_t vd_manifold_hits_ws_bytes(int64_t ns) { return ns < 1 ? 0 : (size_t)ns * sizeof(float); }

extern "C" int vd_manifold_hits_f16(const uint16_t* q, const float* q_sq, int64_t nq, const uint16_t* s, const float* s_sq,
                                    const float* radius, int64_t ns, int32_t d, uint8_t* hit, void* ws, size_t ws_bytes, void* stream) {
    VD_REQUIRE(nq >= 1 && ns >= 1, "vd_manifold_hits_f16: empty set (nq = %lld, ns = %lld)", (long long)nq, (long long)ns);
    VD_REQUIRE(d >= BK && d % BK == 0, "vd_manifold_hits_f16: d = %d is not a positive multiple of %d (pad with zeros)", d, BK);
    VD_REQUIRE(vd_aligned16(q) && vd_aligned16(s), "vd_manifold_hits_f16: q and s must be 16-byte aligned");
    VD_REQUIRE(ws_bytes >= vd_manifold_hits_ws_bytes(ns), "vd_manifold_hits_f16: ws_bytes %zu < %zu", ws_bytes,
               vd_manifold_hits_ws_bytes(ns));
    hipStream_t st = (hipStream_t)stream;
    float* thr = (float*)ws;
    hipLaunchKernelGGL(radius_threshold_kernel, dim3(blocks_for(ns)), dim3(256), 0, st, radius, (long long)ns, thr);
    VD_LAUNCH_CHECK("radius_threshold_kernel");
    VD_REQUIRE(hipMemsetAsync(hit, 0, (size_t)nq, st) == hipSuccess, "vd_manifold_hits_f16: hipMemsetAsync failed");
    KnnArgs a{};
    a.q = q; a.q_sq = q_sq; a.nq = nq; a.c = s; a.c_sq = s_sq; a.nc = ns; a.d = d; a.thr = thr; a.hit = hit;
    a.splits = splits_for(nq, ns); a.nct = (int)((ns + BN - 1) / BN);
    hipLaunchKernelGGL((knn_tile_kernel<4, true>), dim3((unsigned)((nq + BM - 1) / BM), (unsigned)a.splits), dim3(256), 0, st, a);
    VD_LAUNCH_CHECK("knn_tile_kernel<hits>");
    return 0;
}
