// kid.hip -- the two sample-based metrics beside FID: the polynomial-kernel sums of the Kernel Inception Distance (Binkowski et al.
// 2018) and the Inception Score, both in fp64 from fp32 rows, fixed order, no atomics, no n x n buffer.
//
// KID (vd_kid_sums).  For subset s with rows X_s[i] = x[ix[s mx + i]], Y_s[j] = y[iy[s my + j]] and k(a, b) = (gamma <a, b> + coef0)^degree:
//   out[s][0] = sum_{i != j} k(X_s[i], X_s[j]),  out[s][1] = the same over Y_s,  out[s][2] = sum_{i, j} k(X_s[i], Y_s[j]).
// One workgroup of 4 waves owns one 64 x 64 tile of one of the three Gram matrices of one subset across ALL of d (2 x 2 MFMA tiles
// of 16 x 16 per wave on v_mfma_f64_16x16x4_f64, as fid.hip): fp32 features widened to fp64 are multiplied exactly and only the
// sums round.  The tile never leaves the registers: the epilogue forms p = gamma s + coef0 (one multiplication, one addition, not
// fused), raises it by degree - 1 left-to-right multiplications, masks (rows past m; on the diagonal tiles of XX / YY the equal
// POSITIONS i == j -- equal indices at different positions are ordinary pairs), and reduces registers -> lanes -> waves in a fixed
// order to ONE fp64 partial in ws[subset][tile].  XX and YY run the lower triangle of tiles only and double the off-diagonal
// partials (exact: entry (j, i) sums the same exact products in the same order as (i, j)).  A second kernel adds the partials of
// each (subset, Gram) in a fixed order.  Same call -> same bits.
//
// Staging.  The features are row-major with d contiguous and the rows of a tile are gathered, so a thread loads 4 consecutive k of
// ONE row (16 B; the 4 lanes of a row read 64 contiguous bytes) and must write them TRANSPOSED into the K-major LDS tile the MFMA
// operand map wants (A[i = lane & 15][k = lane >> 4]: a wave reads 16 consecutive doubles of 4 consecutive k rows).  Reads are
// ds_read_b64 (64 banks, 32-lane groups): the 80-double pitch of fid.hip (640 B = 128 mod 256) keeps the two k rows of a group on
// disjoint banks.  Writes are ds_write_b64, serviced in 16-LANE groups on 32 banks: a group holds 4 rows x 4 k-quads, and with a
// pitch of 80 doubles (= 0 mod 32 dwords) the four k-quads of a row would fall on the same banks, a 4-way conflict.  So k-quad g
// (k rows 4g .. 4g + 3) is skewed by 4g doubles: a group's 16 doubles then cover all 32 banks once, and because one MFMA step reads
// a single k-quad the skew is a constant inside every read and changes no read's bank spread.  (64 + 12 <= 80: the skew fits the pitch.)
//
// Inception Score (vd_is_scores).  Split k = rows [k n / splits, (k + 1) n / splits).  A workgroup walks a fixed chunk of 64 rows
// of one split, one row at a time: row maximum, Z = sum_c exp(l_c - max) in fp64, p_c = exp(l_c - max) / Z, log p_c = (l_c - max) - log Z;
// it adds p into the chunk's column sums and p log p into the chunk's scalar (0 log 0 = 0) in the workspace.  The second kernel
// adds the chunks in order: S_c = sum_i p_ic, score = exp((sum p log p - sum_c S_c log(S_c / n_k)) / n_k).
#include "common.h"

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int BT = 64;            // tile edge (rows of either set)
constexpr int BK = 16;            // feature columns per step
constexpr int LDT = BT + 16;      // LDS row pitch in doubles
constexpr int TILE = BK * LDT;    // doubles per staged operand tile
constexpr int IS_ROWS = 64;       // rows per Inception Score chunk

struct KidArgs {
    const float* x; const float* y;
    const int32_t* ix; const int32_t* iy;
    long long ldx, ldy;
    int mx, my, d, degree;
    int tx, ty;                    // 64-row tiles of X_s, Y_s
    long long txx, tyy, tiles;     // lower-triangle tile counts of XX, YY; tiles per subset
    double gamma, coef0;
    double* ws; double* out;
};

// k = (gamma s + coef0)^degree, every operation rounded on its own so that a host reference can repeat it
__device__ __forceinline__ double poly_kernel(double s, double gamma, double coef0, int degree) {
#pragma clang fp contract(off)
    double p = gamma * s;
    p = p + coef0;
    double r = p;
    for (int e = 1; e < degree; ++e) r = r * p;
    return r;
}

// linear index t of the lower triangle (row-major: (0,0) (1,0) (1,1) (2,0) ...) -> (ti, tj), tj <= ti
__device__ __forceinline__ void tri_decode(long long t, int& ti, int& tj) {
    long long r = (long long)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while (r * (r + 1) / 2 > t) --r;
    while ((r + 1) * (r + 2) / 2 <= t) ++r;
    ti = (int)r;
    tj = (int)(t - r * (r + 1) / 2);
}

__device__ __forceinline__ void stage_write(double* dst, const f32x4& v) {
#pragma unroll
    for (int q = 0; q < 4; ++q) dst[q * LDT] = (double)v[q];
}

__global__ __launch_bounds__(256) void kid_tile_kernel(const KidArgs p) {
    __shared__ __attribute__((aligned(16))) double smem[2 * 2 * TILE];
    const int subset = blockIdx.y;
    const long long t = blockIdx.x;
    int kind, ti, tj;                                                // 0 = XX, 1 = YY, 2 = XY
    if (t < p.txx) { kind = 0; tri_decode(t, ti, tj); }
    else if (t < p.txx + p.tyy) { kind = 1; tri_decode(t - p.txx, ti, tj); }
    else { kind = 2; const long long u = t - p.txx - p.tyy; ti = (int)(u / p.ty); tj = (int)(u % p.ty); }
    const bool a_is_y = kind == 1, b_is_y = kind != 0;
    const float* const A = a_is_y ? p.y : p.x;
    const float* const B = b_is_y ? p.y : p.x;
    const int32_t* const ia = a_is_y ? p.iy : p.ix;
    const int32_t* const ib = b_is_y ? p.iy : p.ix;
    const long long lda = a_is_y ? p.ldy : p.ldx, ldb = b_is_y ? p.ldy : p.ldx;
    const int ma = a_is_y ? p.my : p.mx, mb = b_is_y ? p.my : p.mx;
    const bool diag = kind < 2 && ti == tj;                          // B tile == A tile
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    const int i0 = ti * BT, j0 = tj * BT;

    // staging: thread -> row tid / 4 of the tile, feature columns 4 (tid % 4) .. + 3 of the step; rows past m are staged as zeros
    const int sr = tid >> 2, kq = tid & 3;
    const bool a_in = i0 + sr < ma, b_in = !diag && j0 + sr < mb;
    const float* pa = A;
    const float* pb = B;
    if (a_in) pa += (long long)(ia ? ia[(long long)subset * ma + i0 + sr] : i0 + sr) * lda + kq * 4;
    if (b_in) pb += (long long)(ib ? ib[(long long)subset * mb + j0 + sr] : j0 + sr) * ldb + kq * 4;
    double* const wdst = smem + kq * 4 * LDT + kq * 4 + sr;          // k-quad kq, skewed by 4 kq doubles

    f64x4 acc[2][2];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int u = 0; u < 2; ++u) acc[s][u] = f64x4{0.0, 0.0, 0.0, 0.0};

    const int steps = p.d / BK;
    const f32x4 zero = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    f32x4 ra = zero, rb = zero;
    if (a_in) ra = *(const f32x4*)pa;
    if (b_in) rb = *(const f32x4*)pb;
    for (int c = 0; c < steps; ++c) {
        // (the buffer written here was last read two steps ago; every wave has passed the barrier of the step between)
        double* const As = smem + (c & 1) * 2 * TILE;
        double* const Bs = diag ? As : As + TILE;
        stage_write(wdst + (c & 1) * 2 * TILE, ra);
        if (!diag) stage_write(wdst + (c & 1) * 2 * TILE + TILE, rb);
        __syncthreads();
        if (c + 1 < steps) {
            if (a_in) ra = *(const f32x4*)(pa + (long long)(c + 1) * BK);
            if (b_in) rb = *(const f32x4*)(pb + (long long)(c + 1) * BK);
        }
#pragma unroll
        for (int kk = 0; kk < BK / 4; ++kk) {
            const int off = (kk * 4 + (lane >> 4)) * LDT + kk * 4 + (lane & 15);
            double a[2], b[2];
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                a[s] = As[off + wm * 32 + s * 16];
                b[s] = Bs[off + wn * 32 + s * 16];
            }
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int u = 0; u < 2; ++u) acc[s][u] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s], b[u], acc[s][u], 0, 0, 0);
        }
    }

    // epilogue: register r of lane l is entry [row (l >> 4) + 4 r][col l & 15] of its 16 x 16 tile.  registers, then lanes, then waves
    double sum = 0.0;
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = i0 + wm * 32 + s * 16 + (lane >> 4) + 4 * r, j = j0 + wn * 32 + u * 16 + (lane & 15);
                const double k = poly_kernel(acc[s][u][r], p.gamma, p.coef0, p.degree);
                sum += (i < ma && j < mb && !(diag && i == j)) ? k : 0.0;
            }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o);
    __syncthreads();                                                 // the last step's operands have been read by every wave
    if (lane == 0) smem[wave] = sum;
    __syncthreads();
    if (tid == 0) {
        const double s4 = ((smem[0] + smem[1]) + smem[2]) + smem[3];
        p.ws[(long long)subset * p.tiles + t] = (kind < 2 && !diag) ? 2.0 * s4 : s4;
    }
}

// out[subset][kind] = the partials of that Gram: thread i adds partials i, i + 256, ... in order, then the 256 sums in a fixed tree
__global__ __launch_bounds__(256) void kid_finish_kernel(const KidArgs p) {
    __shared__ double red[256];
    const int kind = blockIdx.x, subset = blockIdx.y, tid = threadIdx.x;
    const long long lo = kind == 0 ? 0 : (kind == 1 ? p.txx : p.txx + p.tyy);
    const long long hi = kind == 0 ? p.txx : (kind == 1 ? p.txx + p.tyy : p.tiles);
    const double* const w = p.ws + (long long)subset * p.tiles;
    double s = 0.0;
    for (long long i = lo + tid; i < hi; i += 256) s += w[i];
    red[tid] = s;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    if (tid == 0) p.out[subset * 3 + kind] = red[0];
}

// ---------------------------------------------------------------------------------------------------------------- Inception Score
// every thread receives the block's value; waves in order.  red: 4 doubles, free again on return
__device__ __forceinline__ double block_sum(double v, double* red) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    v = ((red[0] + red[1]) + red[2]) + red[3];
    __syncthreads();
    return v;
}

__device__ __forceinline__ float block_max(float v, float* red) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    v = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    return v;
}

__device__ __forceinline__ void split_rows(long long n, int splits, int k, long long& r0, long long& r1) {
    r0 = (long long)k * n / splits;
    r1 = (long long)(k + 1) * n / splits;
}

// ws[split][chunk][0 .. classes - 1] = the chunk's column sums of p, [classes] = its sum of p log p.  Thread t owns columns t, t + 256, ...
__global__ __launch_bounds__(256) void is_rows_kernel(const float* __restrict__ logits, long long n, int classes, long long ld, int splits,
                                                      int chunks, double* __restrict__ ws) {
    __shared__ double redd[4];
    __shared__ float redf[4];
    const int split = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x;
    long long r0, r1;
    split_rows(n, splits, split, r0, r1);
    const long long lo = r0 + (long long)chunk * IS_ROWS;
    if (lo >= r1) return;
    const long long hi = lo + IS_ROWS < r1 ? lo + IS_ROWS : r1;
    double* const cs = ws + ((long long)split * chunks + chunk) * (classes + 1);
    double plp = 0.0;
    for (long long row = lo; row < hi; ++row) {
        const float* const l = logits + row * ld;
        float m = -INFINITY;                                         // fmaxf skips a NaN; the NaN reaches Z through its own exp
        for (int c = tid; c < classes; c += 256) m = fmaxf(m, l[c]);
        const double mx = (double)block_max(m, redf);
        double z = 0.0;
        for (int c = tid; c < classes; c += 256) z += exp((double)l[c] - mx);
        z = block_sum(z, redd);
        const double logz = log(z);
        for (int c = tid; c < classes; c += 256) {
            const double a = (double)l[c] - mx;
            const double pr = exp(a) / z;
            cs[c] = (row == lo ? 0.0 : cs[c]) + pr;
            plp += pr == 0.0 ? 0.0 : pr * (a - logz);                // 0 log 0 = 0; a NaN is not == 0 and stays
        }
    }
    plp = block_sum(plp, redd);
    if (tid == 0) cs[classes] = plp;
}

__global__ __launch_bounds__(256) void is_finish_kernel(long long n, int classes, int splits, int chunks, const double* __restrict__ ws,
                                                        double* __restrict__ scores) {
    __shared__ double redd[4];
    const int split = blockIdx.x, tid = threadIdx.x;
    long long r0, r1;
    split_rows(n, splits, split, r0, r1);
    const double nk = (double)(r1 - r0);
    const int used = (int)((r1 - r0 + IS_ROWS - 1) / IS_ROWS);
    const double* const w = ws + (long long)split * chunks * (classes + 1);
    double cross = 0.0;                                              // sum_c S_c log pbar_c over this thread's columns
    for (int c = tid; c < classes; c += 256) {
        double s = 0.0;
        for (int k = 0; k < used; ++k) s += w[(long long)k * (classes + 1) + c];
        cross += s == 0.0 ? 0.0 : s * log(s / nk);
    }
    cross = block_sum(cross, redd);
    if (tid == 0) {
        double plp = 0.0;
        for (int k = 0; k < used; ++k) plp += w[(long long)k * (classes + 1) + classes];
        scores[split] = exp((plp - cross) / nk);
    }
}

long long tri(long long t) { return t * (t + 1) / 2; }

bool kid_shape(int32_t subsets, int32_t mx, int32_t my) { return subsets >= 1 && subsets <= 65535 && mx >= 2 && my >= 2; }

long long kid_tiles(int32_t mx, int32_t my) {
    const long long tx = ((long long)mx + BT - 1) / BT, ty = ((long long)my + BT - 1) / BT;
    return tri(tx) + tri(ty) + tx * ty;
}

long long is_max_rows(int64_t n, int32_t splits) { return n / splits + (n % splits ? 1 : 0); }

bool is_shape(int64_t n, int32_t classes, int32_t splits) {
    return classes >= 2 && splits >= 1 && splits <= 65535 && n >= splits && n <= ((int64_t)1 << 40);
}

long long is_chunks(int64_t n, int32_t splits) { return (is_max_rows(n, splits) + IS_ROWS - 1) / IS_ROWS; }

}  // namespace

extern "C" size_t vd_kid_ws_bytes(int32_t subsets, int32_t mx, int32_t my) {
    if (!kid_shape(subsets, mx, my)) return 0;
    return (size_t)subsets * (size_t)kid_tiles(mx, my) * sizeof(double);
}

extern "C" int vd_kid_sums(const float* x, int64_t nx, int64_t ldx, const float* y, int64_t ny, int64_t ldy, int32_t d, const int32_t* ix,
                           const int32_t* iy, int32_t subsets, int32_t mx, int32_t my, double gamma, double coef0, int32_t degree,
                           double* out, void* ws, size_t ws_bytes, void* stream) {
    VD_REQUIRE(d >= 16 && d % 16 == 0 && ldx >= d && ldy >= d && ldx % 4 == 0 && ldy % 4 == 0, "vd_kid_sums: d = %d, ldx = %lld, ldy = "
               "%lld (need d a positive multiple of 16, ldx and ldy >= d and multiples of 4)", d, (long long)ldx, (long long)ldy);
    VD_REQUIRE(kid_shape(subsets, mx, my) && mx <= nx && my <= ny, "vd_kid_sums: subsets = %d, mx = %d of nx = %lld, my = %d of ny = "
               "%lld (need 1 <= subsets <= 65535, 2 <= mx <= nx, 2 <= my <= ny)", subsets, mx, (long long)nx, my, (long long)ny);
    VD_REQUIRE(degree >= 1 && degree <= 8, "vd_kid_sums: degree = %d (need 1 <= degree <= 8)", degree);
    VD_REQUIRE((ix || (subsets == 1 && mx == nx)) && (iy || (subsets == 1 && my == ny)), "vd_kid_sums: a null index pointer means the "
               "identity and needs subsets == 1 and m == n (subsets = %d, mx = %d of %lld, my = %d of %lld)", subsets, mx, (long long)nx,
               my, (long long)ny);
    VD_REQUIRE(vd_aligned16(x) && vd_aligned16(y) && vd_aligned16(out) && vd_aligned16(ws), "vd_kid_sums: x, y, out and ws must be "
               "16-byte aligned");
    const long long tiles = kid_tiles(mx, my);
    VD_REQUIRE(tiles <= 0x7fffffffLL, "vd_kid_sums: mx = %d, my = %d make %lld tiles per subset, more than one launch holds", mx, my, tiles);
    VD_REQUIRE(ws_bytes >= vd_kid_ws_bytes(subsets, mx, my), "vd_kid_sums: workspace of %zu bytes, vd_kid_ws_bytes asks for %zu", ws_bytes,
               vd_kid_ws_bytes(subsets, mx, my));
    KidArgs a{};
    a.x = x; a.y = y; a.ix = ix; a.iy = iy; a.ldx = ldx; a.ldy = ldy;
    a.mx = mx; a.my = my; a.d = d; a.degree = degree;
    a.tx = (mx + BT - 1) / BT; a.ty = (my + BT - 1) / BT;
    a.txx = tri(a.tx); a.tyy = tri(a.ty); a.tiles = tiles;
    a.gamma = gamma; a.coef0 = coef0;
    a.ws = (double*)ws; a.out = out;
    hipLaunchKernelGGL(kid_tile_kernel, dim3((unsigned)tiles, (unsigned)subsets), dim3(256), 0, (hipStream_t)stream, a);
    VD_LAUNCH_CHECK("kid_tile_kernel");
    hipLaunchKernelGGL(kid_finish_kernel, dim3(3, (unsigned)subsets), dim3(256), 0, (hipStream_t)stream, a);
    VD_LAUNCH_CHECK("kid_finish_kernel");
    return 0;
}

extern "C" size_t vd_is_ws_bytes(int64_t n, int32_t classes, int32_t splits) {
    if (!is_shape(n, classes, splits)) return 0;
    return (size_t)splits * (size_t)is_chunks(n, splits) * ((size_t)classes + 1) * sizeof(double);
}

extern "C" int vd_is_scores(const float* logits, int64_t n, int32_t classes, int64_t ld, int32_t splits, double* scores, void* ws,
                            size_t ws_bytes, void* stream) {
    VD_REQUIRE(is_shape(n, classes, splits) && ld >= classes, "vd_is_scores: n = %lld, classes = %d, ld = %lld, splits = %d (need classes "
               ">= 2, ld >= classes, 1 <= splits <= 65535 and at least one row per split: splits <= n)", (long long)n, classes,
               (long long)ld, splits);
    VD_REQUIRE(((uintptr_t)logits & 3) == 0 && ((uintptr_t)scores & 7) == 0 && ((uintptr_t)ws & 7) == 0, "vd_is_scores: logits must be "
               "4-byte, scores and ws 8-byte aligned");
    VD_REQUIRE(ws_bytes >= vd_is_ws_bytes(n, classes, splits), "vd_is_scores: workspace of %zu bytes, vd_is_ws_bytes asks for %zu", ws_bytes,
               vd_is_ws_bytes(n, classes, splits));
    const long long chunks = is_chunks(n, splits);
    VD_REQUIRE(chunks <= 0x7fffffffLL, "vd_is_scores: %lld chunks per split, more than one launch holds", chunks);
    hipLaunchKernelGGL(is_rows_kernel, dim3((unsigned)chunks, (unsigned)splits), dim3(256), 0, (hipStream_t)stream, logits, (long long)n,
                       classes, (long long)ld, splits, (int)chunks, (double*)ws);
    VD_LAUNCH_CHECK("is_rows_kernel");
    hipLaunchKernelGGL(is_finish_kernel, dim3((unsigned)splits), dim3(256), 0, (hipStream_t)stream, (long long)n, classes, splits,
                       (int)chunks, (const double*)ws, scores);
    VD_LAUNCH_CHECK("is_finish_kernel");
    return 0;
}
