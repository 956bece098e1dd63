// ba.hip — per-pair normal-equation blocks of the bundle adjustment on gfx950.
//
// Restates the parfor body of accumulateNormalEqnsBlock (PP/bundleAdjustment/bundleAdjustmentRKf.m:717-741) with
// jacobianPair (:793-899), computeSingleResidual (:1641-1686), computeJacobianWrtCamera (:1688-1783) and huberWeight
// (:1806-1829): for every matched pair of images the blocks Hii = Ji'Ji, Hjj = Jj'Jj, Hij = Ji'Jj, gi = Ji'r, gj = Jj'r
// and the energy / residual statistics.  The resident problem (aps_ba_problem_create / aps_ba_normal_eqns, end of file)
// also assembles the dense H and g on the device; the LM loop, the prior and the solve stay on the host.
//
// All arithmetic is f64 in the order fixed by oracle/ba_oracle.c (matrix chains left to right as written in the
// reference, inner index ascending, no fma; per-pair sums as 64 lane-strided partials + xor butterfly), so the blocks
// are bit-identical to the oracle's.  One wavefront per pair: the ten 3x3 matrices of a direction depend on the pair
// only and are computed once per lane (uniformly), a lane then walks its matches with a handful of mat-vecs each.
// Neither bound is in sight (<= 10^9 flop for the 64-view scene); the point is to take 384 pairs x 4 k matches x
// ~50 LM evaluations of interpreted per-match loops off the host.
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "aps_internal.h"

namespace aps {

struct BaCam {
    double f, cx, cy;
    double R[9];  // column-major
};

#define M3(A, r, c) (A)[(r) + 3 * (c)]

__device__ __forceinline__ void mul33(const double* A, const double* B, double* C) {
    double T[9];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            double s = M3(A, r, 0) * M3(B, 0, c);
            s = s + M3(A, r, 1) * M3(B, 1, c);
            s = s + M3(A, r, 2) * M3(B, 2, c);
            M3(T, r, c) = s;
        }
#pragma unroll
    for (int e = 0; e < 9; ++e) C[e] = T[e];
}

__device__ __forceinline__ void mulv(const double* A, const double* x, double* y) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        double s = M3(A, r, 0) * x[0];
        s = s + M3(A, r, 1) * x[1];
        s = s + M3(A, r, 2) * x[2];
        y[r] = s;
    }
}

__device__ __forceinline__ void kmat(const BaCam& c, double* K) {
#pragma unroll
    for (int e = 0; e < 9; ++e) K[e] = 0.0;
    M3(K, 0, 0) = c.f;
    M3(K, 1, 1) = c.f;
    M3(K, 0, 2) = c.cx;
    M3(K, 1, 2) = c.cy;
    M3(K, 2, 2) = 1.0;
}

__device__ __forceinline__ void skew_unit(int m, double* S) {
#pragma unroll
    for (int e = 0; e < 9; ++e) S[e] = 0.0;
    const double v0 = m == 0 ? 1.0 : 0.0, v1 = m == 1 ? 1.0 : 0.0, v2 = m == 2 ? 1.0 : 0.0;
    M3(S, 0, 1) = -v2;
    M3(S, 0, 2) = v1;
    M3(S, 1, 0) = v2;
    M3(S, 1, 2) = -v0;
    M3(S, 2, 0) = -v1;
    M3(S, 2, 1) = v0;
}

__device__ __forceinline__ void ksolve(const BaCam& c, double x, double y, double* out) {
    const double z = 1.0;
    out[2] = z;
    out[1] = (y - c.cy * z) / c.f;
    out[0] = (x - c.cx * z) / c.f;
}

// K_obs R_obs R_src' of the incremented cameras: the matrix of the residual (computeSingleResidual :1668-1680)
__device__ __forceinline__ void make_ml(const BaCam& ol, const BaCam& sl, double* ML) {
    double K[9], A[9], RsT[9];
    kmat(ol, K);
    mul33(K, ol.R, A);
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) M3(RsT, c, r) = M3(sl.R, r, c);
    mul33(A, RsT, ML);
}

struct DirMats {
    double M[9], G[3][9], N[3][9], D[9], Q[9], ML[9];
};

__device__ void make_dir(const BaCam& ob, const BaCam& sb, const BaCam& ol, const BaCam& sl, DirMats& d) {
    double K[9], A[9], RsT[9], S[9], T[9], nR[9];
    kmat(ob, K);
    mul33(K, ob.R, A);
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) M3(RsT, c, r) = M3(sb.R, r, c);
    mul33(A, RsT, d.M);
#pragma unroll
    for (int e = 0; e < 9; ++e) nR[e] = -RsT[e];
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        skew_unit(m, S);
        mul33(A, S, T);
        mul33(T, RsT, d.G[m]);
        mul33(nR, S, T);
        mul33(A, T, d.N[m]);
    }
    double dK[9] = {1, 0, 0, 0, 1, 0, 0, 0, 0};
    mul33(dK, ob.R, T);
    mul33(T, RsT, d.D);
    const double f = sb.f;
    double dKi[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) dKi[e] = 0.0;
    M3(dKi, 0, 0) = -1.0 / (f * f);
    M3(dKi, 1, 1) = -1.0 / (f * f);
    M3(dKi, 0, 2) = sb.cx / (f * f);
    M3(dKi, 1, 2) = sb.cy / (f * f);
    mul33(d.M, dKi, d.Q);
    make_ml(ol, sl, d.ML);
}

__device__ __forceinline__ double one_direction(const DirMats& d, const BaCam& sb, const BaCam& sl, double uox, double uoy,
                                                double usx, double usy, double sigma, double* r, double Jobs[2][4],
                                                double Jsrc[2][4]) {
    double xb[3], pH[3], v[3];
    ksolve(sb, usx, usy, xb);
    mulv(d.M, xb, pH);
    const double x = pH[0], y = pH[1];
    double z = pH[2];
    if (fabs(z) < 1e-10) z = 1e-10;
    const double iz = 1.0 / z, zz = z * z;
    const double a = -iz, cx_ = x / zz, cy_ = y / zz;
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        mulv(d.G[m], xb, v);
        Jobs[0][m] = a * v[0] + cx_ * v[2];
        Jobs[1][m] = a * v[1] + cy_ * v[2];
        mulv(d.N[m], xb, v);
        Jsrc[0][m] = a * v[0] + cx_ * v[2];
        Jsrc[1][m] = a * v[1] + cy_ * v[2];
    }
    mulv(d.D, xb, v);
    Jobs[0][3] = a * v[0] + cx_ * v[2];
    Jobs[1][3] = a * v[1] + cy_ * v[2];
    const double uh[3] = {usx, usy, 1.0};
    mulv(d.Q, uh, v);
    Jsrc[0][3] = a * v[0] + cx_ * v[2];
    Jsrc[1][3] = a * v[1] + cy_ * v[2];
    double xl[3], pL[3];
    ksolve(sl, usx, usy, xl);
    mulv(d.ML, xl, pL);
    double zl = pL[2];
    if (fabs(zl) < 1e-10) zl = 1e-10;
    const double r0 = uox - pL[0] / zl, r1 = uoy - pL[1] / zl;
    const double rr = r0 * r0 + r1 * r1;
    const double nr = sqrt(rr);
    const double w = nr < sigma ? 1.0 : sigma / nr;
    const double sw = sqrt(w);
    r[0] = sw * r0;
    r[1] = sw * r1;
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            Jobs[q][e] = sw * Jobs[q][e];
            Jsrc[q][e] = sw * Jsrc[q][e];
        }
    return (sw * sw) * rr;
}

constexpr int kBaAcc = 59;  // Hii 16, Hjj 16, Hij 16 (column-major 4x4), gi 4, gj 4, E, r2sum, rcnt

__device__ __forceinline__ void add_rows(double* acc, const double* r, double Ji[2][4], double Jj[2][4]) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                acc[a + 4 * b] = acc[a + 4 * b] + Ji[q][a] * Ji[q][b];
                acc[16 + a + 4 * b] = acc[16 + a + 4 * b] + Jj[q][a] * Jj[q][b];
                acc[32 + a + 4 * b] = acc[32 + a + 4 * b] + Ji[q][a] * Jj[q][b];
            }
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            acc[48 + a] = acc[48 + a] + Ji[q][a] * r[q];
            acc[52 + a] = acc[52 + a] + Jj[q][a] * r[q];
        }
    }
}

// The residual alone (the tail of one_direction, same operations in the same order): the weighted squared norm of the
// energy-only evaluation.
__device__ __forceinline__ double residual_only(const double* ML, const BaCam& sl, double uox, double uoy, double usx,
                                                double usy, double sigma) {
    double xl[3], pL[3];
    ksolve(sl, usx, usy, xl);
    mulv(ML, xl, pL);
    double zl = pL[2];
    if (fabs(zl) < 1e-10) zl = 1e-10;
    const double r0 = uox - pL[0] / zl, r1 = uoy - pL[1] / zl;
    const double rr = r0 * r0 + r1 * r1;
    const double nr = sqrt(rr);
    const double w = nr < sigma ? 1.0 : sigma / nr;
    const double sw = sqrt(w);
    return (sw * sw) * rr;
}

// One pair on one wavefront: c = (base i, base j, incremented i, incremented j), matches r0 .. r0+m-1 of Ui / Uj.
// kFull: the 59 accumulators; otherwise only E, r2sum, rcnt (out[56..58]), summed exactly as in the full form.
template <bool kFull>
__device__ __forceinline__ void pair_blocks_wave(const BaCam* c, const double* __restrict__ Ui, const double* __restrict__ Uj,
                                                 int64_t ldu, int64_t r0, int64_t m, double sigma, int both,
                                                 double* __restrict__ out) {
    const int lane = threadIdx.x;
    if constexpr (kFull) {
        // the direction matrices live in LDS (two x 90 doubles): every lane computes the same values, lane 0's copy is kept
        __shared__ DirMats s_dir[2];
        if (lane == 0) {
            make_dir(c[0], c[1], c[2], c[3], s_dir[0]);  // j -> i: observed in i, source j
            make_dir(c[1], c[0], c[3], c[2], s_dir[1]);  // i -> j
        }
        __syncthreads();
        double acc[kBaAcc];
#pragma unroll
        for (int e = 0; e < kBaAcc; ++e) acc[e] = 0.0;
        for (int64_t k = lane; k < m; k += 64) {
            const double uix = Ui[r0 + k], uiy = Ui[ldu + r0 + k], ujx = Uj[r0 + k], ujy = Uj[ldu + r0 + k];
            double r[2], Jo[2][4], Js[2][4];
            double wr = one_direction(s_dir[0], c[1], c[3], uix, uiy, ujx, ujy, sigma, r, Jo, Js);
            add_rows(acc, r, Jo, Js);
            acc[56] = acc[56] + 0.5 * wr;
            acc[57] = acc[57] + wr;
            acc[58] = acc[58] + 2.0;
            if (both) {
                wr = one_direction(s_dir[1], c[0], c[2], ujx, ujy, uix, uiy, sigma, r, Jo, Js);
                add_rows(acc, r, Js, Jo);
                acc[56] = acc[56] + 0.5 * wr;
                acc[57] = acc[57] + wr;
                acc[58] = acc[58] + 2.0;
            }
        }
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) {
#pragma unroll
            for (int e = 0; e < kBaAcc; ++e) acc[e] = acc[e] + __shfl_xor(acc[e], s);
        }
        if (lane == 0)
            for (int e = 0; e < kBaAcc; ++e) out[e] = acc[e];
    } else {
        __shared__ double s_ml[2][9];
        if (lane == 0) {
            make_ml(c[2], c[3], s_ml[0]);
            make_ml(c[3], c[2], s_ml[1]);
        }
        __syncthreads();
        double acc[3] = {0.0, 0.0, 0.0};
        for (int64_t k = lane; k < m; k += 64) {
            const double uix = Ui[r0 + k], uiy = Ui[ldu + r0 + k], ujx = Uj[r0 + k], ujy = Uj[ldu + r0 + k];
            double wr = residual_only(s_ml[0], c[3], uix, uiy, ujx, ujy, sigma);
            acc[0] = acc[0] + 0.5 * wr;
            acc[1] = acc[1] + wr;
            acc[2] = acc[2] + 2.0;
            if (both) {
                wr = residual_only(s_ml[1], c[2], ujx, ujy, uix, uiy, sigma);
                acc[0] = acc[0] + 0.5 * wr;
                acc[1] = acc[1] + wr;
                acc[2] = acc[2] + 2.0;
            }
        }
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) {
#pragma unroll
            for (int e = 0; e < 3; ++e) acc[e] = acc[e] + __shfl_xor(acc[e], s);
        }
        if (lane == 0)
            for (int e = 0; e < 3; ++e) out[56 + e] = acc[e];
    }
}

__device__ __forceinline__ void load_cam(const double* s, BaCam& c) {
    c.f = s[0];
    c.cx = s[1];
    c.cy = s[2];
#pragma unroll
    for (int e = 0; e < 9; ++e) c.R[e] = s[3 + e];
}

__global__ __launch_bounds__(64) void ba_pair_blocks_kernel(const double* __restrict__ Ui, const double* __restrict__ Uj,
                                                           int64_t ldu, const int64_t* __restrict__ pair_ptr,
                                                           const double* __restrict__ cams, double sigma, int both,
                                                           double* __restrict__ out) {
    const int p = blockIdx.x;
    BaCam c[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) load_cam(cams + ((int64_t)p * 4 + q) * 12, c[q]);
    const int64_t r0 = pair_ptr[p], m = pair_ptr[p + 1] - r0;
    pair_blocks_wave<true>(c, Ui, Uj, ldu, r0, m, sigma, both, out + (int64_t)p * kBaAcc);
}

// ---- the resident problem (aps_ba_problem_create / aps_ba_normal_eqns) ----------------------------------------------------
//
// A pair is live in an evaluation when both its cameras have a column (col_start >= 0) and it has matches: exactly the pairs
// the host loop of accumulateNormalEqnsBlock visits for a sorted camList.  The blocks kernel leaves the other records alone;
// the assembly reads only live ones.

__device__ __forceinline__ bool pair_live(int p, const int* __restrict__ ij, const int64_t* __restrict__ ptr,
                                          const int* __restrict__ col_start) {
    return col_start[ij[2 * p]] >= 0 && col_start[ij[2 * p + 1]] >= 0 && ptr[p + 1] > ptr[p];
}

template <bool kFull>
__global__ __launch_bounds__(64) void ba_problem_blocks_kernel(const double* __restrict__ Ui, const double* __restrict__ Uj,
                                                              int64_t ldu, const int64_t* __restrict__ pair_ptr,
                                                              const int* __restrict__ ij, const double* __restrict__ base,
                                                              const double* __restrict__ lin, const int* __restrict__ col_start,
                                                              double sigma, int both, double* __restrict__ out) {
    const int p = blockIdx.x;
    if (!pair_live(p, ij, pair_ptr, col_start)) return;  // uniform over the wave
    const int i = ij[2 * p], j = ij[2 * p + 1];
    BaCam c[4];
    load_cam(base + (int64_t)i * 12, c[0]);
    load_cam(base + (int64_t)j * 12, c[1]);
    load_cam(lin + (int64_t)i * 12, c[2]);
    load_cam(lin + (int64_t)j * 12, c[3]);
    const int64_t r0 = pair_ptr[p], m = pair_ptr[p + 1] - r0;
    pair_blocks_wave<kFull>(c, Ui, Uj, ldu, r0, m, sigma, both, out + (int64_t)p * kBaAcc);
}

// The serial reduction of accumulateNormalEqnsBlock (:743-789) as the host mirror does it (bundleAdjustment.py): every cell
// of H and of g starts at +0.0 and takes its blocks in pair order.  Workgroup k < n_cams writes the whole column strip of
// camera k (H is column-major, P x P): its diagonal block and g entries walk k's pair list (ascending (i, j)), an
// off-diagonal cell comes from the one pair of the two cameras (0.0 + x), every other cell is 0.0.  The last workgroup sums
// E, r2sum and rcnt over the live pairs in pair order on one lane.  out = [E r2sum rcnt | g (P) | H (P x P)].
__global__ __launch_bounds__(256) void ba_assemble_kernel(const double* __restrict__ blocks, const int* __restrict__ ij,
                                                          const int64_t* __restrict__ pair_ptr, const int* __restrict__ cam_ptr,
                                                          const int* __restrict__ cam_list, const int* __restrict__ pair_of,
                                                          const int* __restrict__ col_start, const int* __restrict__ n_params,
                                                          const int* __restrict__ row_cam, int n_cams, int n_pairs, int P,
                                                          double* __restrict__ out) {
    const int tid = threadIdx.x;
    if ((int)blockIdx.x == (int)gridDim.x - 1) {
        if (tid == 0) {
            double E = 0.0, R2 = 0.0, cnt = 0.0;
            for (int p = 0; p < n_pairs; ++p) {
                if (!pair_live(p, ij, pair_ptr, col_start)) continue;
                const double* o = blocks + (int64_t)p * kBaAcc;
                E = E + o[56];
                R2 = R2 + o[57];
                cnt = cnt + o[58];
            }
            out[0] = E;
            out[1] = R2;
            out[2] = cnt;
        }
        return;
    }
    const int k = blockIdx.x;
    const int c0 = col_start[k];
    if (c0 < 0) return;
    const int nk = n_params[k];
    double* g = out + 3;
    double* H = out + 3 + P;
    const int q0 = cam_ptr[k], q1 = cam_ptr[k + 1];
    if (tid < nk) {
        double s = 0.0;
        for (int q = q0; q < q1; ++q) {
            const int p = cam_list[q] >> 1, role = cam_list[q] & 1;
            if (!pair_live(p, ij, pair_ptr, col_start)) continue;
            s = s + blocks[(int64_t)p * kBaAcc + 48 + 4 * role + tid];
        }
        g[c0 + tid] = s;
    }
    for (int idx = tid; idx < nk * P; idx += 256) {
        const int b = idx / P, r = idx - b * P;
        const int m = row_cam[r], a = r - col_start[m];
        double v = 0.0;
        if (m == k) {
            for (int q = q0; q < q1; ++q) {
                const int p = cam_list[q] >> 1, role = cam_list[q] & 1;
                if (!pair_live(p, ij, pair_ptr, col_start)) continue;
                v = v + blocks[(int64_t)p * kBaAcc + 16 * role + a + 4 * b];
            }
        } else {
            const int lo = m < k ? m : k, hi = m < k ? k : m;
            const int p = pair_of[(int64_t)lo * n_cams + hi];
            if (p >= 0 && pair_ptr[p + 1] > pair_ptr[p]) {
                // Hij is (params of i) x (params of j): row a of camera m = i and column b of k = j, or the transpose
                const double x = blocks[(int64_t)p * kBaAcc + 32 + (k == hi ? a + 4 * b : b + 4 * a)];
                v = 0.0 + x;
            }
        }
        H[(int64_t)(c0 + b) * P + r] = v;
    }
}

// ---- bundleAdjustmentH: the one-direction data term of residualsJacobian (aps_ba_h_normal_eqns) ---------------------------
//
// PP/bundleAdjustment/bundleAdjustmentH.m:282-436 with computeUnidirResiduals (:512-590) and computeJacobianBatch (:685-737).
// Match k of pair (i, j): Y = H [u v 1]' as Y1 = (a u + b v) + c, Y2 = (d u + e v) + f, Y3 = (g u + h v) + 1 (H(3,3) = 1),
// res = Yi(1:2) / Yi3 - Yj(1:2) / Yj3, the Huber weight w = delta / |res| when |res| >= delta > 0 (else 1) multiplies res
// itself, and the two rows of a side are ((dY/dp) Y3 - Y (dY3/dp)) / (Y3 Y3) * w, those of Hj negated.  Written out, a
// side's rows carry seven distinct values: row u = [A0 A1 A2 0 0 0 Bu0 Bu1], row v = [0 0 0 A0 A1 A2 Bv0 Bv1] with
// A = ([u v 1] Y3 - Y1 0) / Y3^2 w, Bu = (0 Y3 - Y1 [u v]) / Y3^2 w, Bv = (0 Y3 - Y2 [u v]) / Y3^2 w.  The literal row v
// value of A differs from row u's at most in the sign of a zero, and a product with a +-0 factor leaves an accumulator
// unchanged (every accumulator starts at +0.0, so none is ever -0.0): the compact sums below equal the literal
// sum over both rows of J'J and J'r bit for bit (finite inputs).  Each cell takes, match by match, the row u term then
// the row v term; per pair 64 lane-strided partials and an xor butterfly, as in the RKf blocks.
//
// Three waves per pair (blockIdx.y): part 0 = Hii, gi and the sums, part 1 = Hjj and gj, part 2 = Hij; part 3 (the energy-only
// launch) = the sums alone, computed by the same code as part 0.  Record per pair (kBaHRec f64): Hii, Hjj, Hij (8 x 8
// column-major), gi, gj (8), then sum (w res)^2, sum |res|^2, match count.

constexpr int kBaHRec = 3 * 64 + 16 + 3;
constexpr int kHSide = 29;   // AA 6 (symmetric), A Bu 6, A Bv 6, BB 3 (symmetric), g: A ru 3, A rv 3, B 2
constexpr int kHCross = 37;  // Ai Aj 9, Ai Buj 6, Ai Bvj 6, Bui Aj 6, Bvi Aj 6, BBij 4

struct HSide {
    double A[3], Bu[2], Bv[2];
};

__device__ __forceinline__ constexpr int sym3(int a, int b) {
    return a <= b ? (a == 0 ? b : a == 1 ? 2 + b : 5) : (b == 0 ? a : b == 1 ? 2 + a : 5);
}

__device__ __forceinline__ constexpr int sym2(int a, int b) { return a + b; }

__device__ __forceinline__ void h_project(const double* Hm, double u, double v, double& Y1, double& Y2, double& Y3) {
    Y1 = Hm[0] * u + Hm[1] * v + Hm[2];
    Y2 = Hm[3] * u + Hm[4] * v + Hm[5];
    Y3 = Hm[6] * u + Hm[7] * v + 1.0;
}

__device__ __forceinline__ void h_side(double u, double v, double Y1, double Y2, double Y3, double w, bool negate, HSide& s) {
    const double y3sq = Y3 * Y3;
    const double z = 0.0 * Y3;
    const double d[3] = {u, v, 1.0};
#pragma unroll
    for (int a = 0; a < 3; ++a) s.A[a] = (d[a] * Y3 - Y1 * 0.0) / y3sq * w;
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        s.Bu[b] = (z - Y1 * d[b]) / y3sq * w;
        s.Bv[b] = (z - Y2 * d[b]) / y3sq * w;
    }
    if (negate) {
#pragma unroll
        for (int a = 0; a < 3; ++a) s.A[a] = -s.A[a];
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            s.Bu[b] = -s.Bu[b];
            s.Bv[b] = -s.Bv[b];
        }
    }
}

__device__ __forceinline__ void h_side_acc(double* acc, const HSide& s, double wru, double wrv) {
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = a; b < 3; ++b) acc[sym3(a, b)] = acc[sym3(a, b)] + s.A[a] * s.A[b];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            acc[6 + 2 * a + b] = acc[6 + 2 * a + b] + s.A[a] * s.Bu[b];
            acc[12 + 2 * a + b] = acc[12 + 2 * a + b] + s.A[a] * s.Bv[b];
        }
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = a; b < 2; ++b) {
            acc[18 + sym2(a, b)] = acc[18 + sym2(a, b)] + s.Bu[a] * s.Bu[b];
            acc[18 + sym2(a, b)] = acc[18 + sym2(a, b)] + s.Bv[a] * s.Bv[b];
        }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        acc[21 + a] = acc[21 + a] + s.A[a] * wru;
        acc[24 + a] = acc[24 + a] + s.A[a] * wrv;
    }
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        acc[27 + b] = acc[27 + b] + s.Bu[b] * wru;
        acc[27 + b] = acc[27 + b] + s.Bv[b] * wrv;
    }
}

__device__ __forceinline__ void h_cross_acc(double* acc, const HSide& si, const HSide& sj) {
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) acc[3 * a + b] = acc[3 * a + b] + si.A[a] * sj.A[b];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            acc[9 + 2 * a + b] = acc[9 + 2 * a + b] + si.A[a] * sj.Bu[b];
            acc[15 + 2 * a + b] = acc[15 + 2 * a + b] + si.A[a] * sj.Bv[b];
        }
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            acc[21 + 3 * a + b] = acc[21 + 3 * a + b] + si.Bu[a] * sj.A[b];
            acc[27 + 3 * a + b] = acc[27 + 3 * a + b] + si.Bv[a] * sj.A[b];
        }
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            acc[33 + 2 * a + b] = acc[33 + 2 * a + b] + si.Bu[a] * sj.Bu[b];
            acc[33 + 2 * a + b] = acc[33 + 2 * a + b] + si.Bv[a] * sj.Bv[b];
        }
}

// the 8 x 8 block (column-major) and the 8 g entries of one side from its compact sums; structural zeros are +0.0
__device__ __forceinline__ void h_side_write(const double* acc, double* Hb, double* gb) {
    static_for<0, 64>([&](auto e) {
        constexpr int a = e % 8, b = e / 8;
        constexpr int ga = a < 3 ? 0 : a < 6 ? 1 : 2, gb_ = b < 3 ? 0 : b < 6 ? 1 : 2;
        double v = 0.0;
        if constexpr (ga == gb_ && ga < 2) v = acc[sym3(a - 3 * ga, b - 3 * gb_)];
        else if constexpr (ga == 0 && gb_ == 2) v = acc[6 + 2 * a + (b - 6)];
        else if constexpr (ga == 2 && gb_ == 0) v = acc[6 + 2 * b + (a - 6)];
        else if constexpr (ga == 1 && gb_ == 2) v = acc[12 + 2 * (a - 3) + (b - 6)];
        else if constexpr (ga == 2 && gb_ == 1) v = acc[12 + 2 * (b - 3) + (a - 6)];
        else if constexpr (ga == 2 && gb_ == 2) v = acc[18 + sym2(a - 6, b - 6)];
        Hb[e] = v;
    });
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        gb[a] = acc[21 + a];
        gb[3 + a] = acc[24 + a];
    }
    gb[6] = acc[27];
    gb[7] = acc[28];
}

__device__ __forceinline__ void h_cross_write(const double* acc, double* Hb) {
    static_for<0, 64>([&](auto e) {
        constexpr int a = e % 8, b = e / 8;  // a: parameter of i (row), b: parameter of j (column)
        constexpr int ga = a < 3 ? 0 : a < 6 ? 1 : 2, gb_ = b < 3 ? 0 : b < 6 ? 1 : 2;
        double v = 0.0;
        if constexpr (ga == gb_ && ga < 2) v = acc[3 * (a - 3 * ga) + (b - 3 * gb_)];
        else if constexpr (ga == 0 && gb_ == 2) v = acc[9 + 2 * a + (b - 6)];
        else if constexpr (ga == 1 && gb_ == 2) v = acc[15 + 2 * (a - 3) + (b - 6)];
        else if constexpr (ga == 2 && gb_ == 0) v = acc[21 + 3 * (a - 6) + b];
        else if constexpr (ga == 2 && gb_ == 1) v = acc[27 + 3 * (a - 6) + (b - 3)];
        else if constexpr (ga == 2 && gb_ == 2) v = acc[33 + 2 * (a - 6) + (b - 6)];
        Hb[e] = v;
    });
}

template <int kPart>
__device__ __forceinline__ void h_pair_part(const double* hi, const double* hj, const double* __restrict__ Ui,
                                            const double* __restrict__ Uj, int64_t ldu, int64_t r0, int64_t m, double delta,
                                            double* __restrict__ rec) {
    constexpr bool kSums = kPart == 0 || kPart == 3;
    constexpr int kBody = kPart == 0 ? kHSide : kPart == 1 ? kHSide : kPart == 2 ? kHCross : 0;
    constexpr int kN = kBody + (kSums ? 3 : 0);
    const int lane = threadIdx.x;
    double acc[kN];
#pragma unroll
    for (int e = 0; e < kN; ++e) acc[e] = 0.0;
    for (int64_t k = lane; k < m; k += 64) {
        const double ui = Ui[r0 + k], vi = Ui[ldu + r0 + k], uj = Uj[r0 + k], vj = Uj[ldu + r0 + k];
        double Yi1, Yi2, Yi3, Yj1, Yj2, Yj3;
        h_project(hi, ui, vi, Yi1, Yi2, Yi3);
        h_project(hj, uj, vj, Yj1, Yj2, Yj3);
        const double ru = Yi1 / Yi3 - Yj1 / Yj3, rv = Yi2 / Yi3 - Yj2 / Yj3;
        const double nn = ru * ru + rv * rv;
        double w = 1.0;
        if (delta > 0.0) {
            const double n = sqrt(nn);
            if (n >= delta) w = delta / n;
        }
        const double wru = ru * w, wrv = rv * w;
        if constexpr (kSums) {
            acc[kBody] = acc[kBody] + wru * wru;
            acc[kBody] = acc[kBody] + wrv * wrv;
            acc[kBody + 1] = acc[kBody + 1] + nn;
            acc[kBody + 2] = acc[kBody + 2] + 1.0;
        }
        if constexpr (kPart == 0 || kPart == 2) {
            HSide si;
            h_side(ui, vi, Yi1, Yi2, Yi3, w, false, si);
            if constexpr (kPart == 0) {
                h_side_acc(acc, si, wru, wrv);
            } else {
                HSide sj;
                h_side(uj, vj, Yj1, Yj2, Yj3, w, true, sj);
                h_cross_acc(acc, si, sj);
            }
        } else if constexpr (kPart == 1) {
            HSide sj;
            h_side(uj, vj, Yj1, Yj2, Yj3, w, true, sj);
            h_side_acc(acc, sj, wru, wrv);
        }
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
#pragma unroll
        for (int e = 0; e < kN; ++e) acc[e] = acc[e] + __shfl_xor(acc[e], s);
    }
    if (lane != 0) return;
    if constexpr (kPart == 0) h_side_write(acc, rec, rec + 192);
    if constexpr (kPart == 1) h_side_write(acc, rec + 64, rec + 200);
    if constexpr (kPart == 2) h_cross_write(acc, rec + 128);
    if constexpr (kSums) {
        rec[208] = acc[kBody];
        rec[209] = acc[kBody + 1];
        rec[210] = acc[kBody + 2];
    }
}

// kFull: grid (n_pairs, 3), one part per wave; otherwise grid (n_pairs, 1), the sums only.  Pairs without matches are left
// alone (the assembly skips them).  G: n_cams x 9 row-major, G[9 k + 8] = 1.
template <bool kFull>
__global__ __launch_bounds__(64) void ba_h_blocks_kernel(const double* __restrict__ Ui, const double* __restrict__ Uj,
                                                        int64_t ldu, const int64_t* __restrict__ pair_ptr,
                                                        const int* __restrict__ ij, const double* __restrict__ G, double delta,
                                                        double* __restrict__ out) {
    const int p = blockIdx.x;
    const int64_t r0 = pair_ptr[p], m = pair_ptr[p + 1] - r0;
    if (m <= 0) return;  // uniform over the wave
    double hi[8], hj[8];
    const double* gi = G + (int64_t)ij[2 * p] * 9;
    const double* gj = G + (int64_t)ij[2 * p + 1] * 9;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        hi[e] = gi[e];
        hj[e] = gj[e];
    }
    double* rec = out + (int64_t)p * kBaHRec;
    if constexpr (kFull) {
        if (blockIdx.y == 0)
            h_pair_part<0>(hi, hj, Ui, Uj, ldu, r0, m, delta, rec);
        else if (blockIdx.y == 1)
            h_pair_part<1>(hi, hj, Ui, Uj, ldu, r0, m, delta, rec);
        else
            h_pair_part<2>(hi, hj, Ui, Uj, ldu, r0, m, delta, rec);
    } else {
        h_pair_part<3>(hi, hj, Ui, Uj, ldu, r0, m, delta, rec);
    }
}

// The dense assembly of the data term, in the host mirror's order (bundleAdjustment.py, hNormalEqnsMirror): every cell of
// H and g starts at +0.0 and takes its blocks in ascending (i, j) pair order.  Workgroup k < n_cams writes the column strip
// of image k unless k is the seed (col_start[k] = -1): its diagonal block and g walk k's pair list (a pair with the seed
// adds there too), an off-diagonal cell is 0.0 + x from the one pair of the two images, every other cell 0.0.  The last
// workgroup sums the three statistics over the pairs with matches, in pair order, on one lane.
// out = [sum (w res)^2, sum |res|^2, count | g (P) | H (P x P)].
__global__ __launch_bounds__(256) void ba_h_assemble_kernel(const double* __restrict__ blocks, const int* __restrict__ ij,
                                                            const int64_t* __restrict__ pair_ptr, const int* __restrict__ cam_ptr,
                                                            const int* __restrict__ cam_list, const int* __restrict__ pair_of,
                                                            const int* __restrict__ col_start, const int* __restrict__ blk_cam,
                                                            int n_cams, int n_pairs, int P, double* __restrict__ out) {
    const int tid = threadIdx.x;
    if ((int)blockIdx.x == (int)gridDim.x - 1) {
        if (tid == 0) {
            double s0 = 0.0, s1 = 0.0, s2 = 0.0;
            for (int p = 0; p < n_pairs; ++p) {
                if (pair_ptr[p + 1] <= pair_ptr[p]) continue;
                const double* o = blocks + (int64_t)p * kBaHRec;
                s0 = s0 + o[208];
                s1 = s1 + o[209];
                s2 = s2 + o[210];
            }
            out[0] = s0;
            out[1] = s1;
            out[2] = s2;
        }
        return;
    }
    const int k = blockIdx.x;
    const int c0 = col_start[k];
    if (c0 < 0) return;
    double* g = out + 3;
    double* H = out + 3 + P;
    const int q0 = cam_ptr[k], q1 = cam_ptr[k + 1];
    if (tid < 8) {
        double s = 0.0;
        for (int q = q0; q < q1; ++q) {
            const int p = cam_list[q] >> 1, role = cam_list[q] & 1;
            if (pair_ptr[p + 1] <= pair_ptr[p]) continue;
            s = s + blocks[(int64_t)p * kBaHRec + 192 + 8 * role + tid];
        }
        g[c0 + tid] = s;
    }
    for (int idx = tid; idx < 8 * P; idx += 256) {
        const int b = idx / P, r = idx - b * P;
        const int m = blk_cam[r >> 3], a = r & 7;
        double v = 0.0;
        if (m == k) {
            for (int q = q0; q < q1; ++q) {
                const int p = cam_list[q] >> 1, role = cam_list[q] & 1;
                if (pair_ptr[p + 1] <= pair_ptr[p]) continue;
                v = v + blocks[(int64_t)p * kBaHRec + 64 * role + a + 8 * b];
            }
        } else {
            const int lo = m < k ? m : k, hi = m < k ? k : m;
            const int p = pair_of[(int64_t)lo * n_cams + hi];
            if (p >= 0 && pair_ptr[p + 1] > pair_ptr[p]) {
                // Hij is (params of i) x (params of j): row a of image m = i and column b of k = j, or the transpose
                const double x = blocks[(int64_t)p * kBaHRec + 128 + (k == hi ? a + 8 * b : b + 8 * a)];
                v = 0.0 + x;
            }
        }
        H[(int64_t)(c0 + b) * P + r] = v;
    }
}

}  // namespace aps

using namespace aps;

extern "C" int aps_ba_pair_blocks(const double* Ui, const double* Uj, int64_t ldu, const int64_t* pair_ptr, int n_pairs,
                                  const double* cams, double sigma_huber, int both_directions, double* out) {
    return guarded([&] {
        APS_REQUIRE(n_pairs >= 0, APS_E_ARG, "negative pair count");
        if (n_pairs == 0) return;
        APS_REQUIRE(Ui && Uj && pair_ptr && cams && out, APS_E_ARG, "NULL argument");
        APS_REQUIRE(sigma_huber > 0.0 && std::isfinite(sigma_huber), APS_E_ARG, "sigmaHuber must be positive and finite");
        ctx();
        std::vector<int64_t> hp(n_pairs + 1);
        const bool dev_ptr = is_device_ptr(pair_ptr);
        if (dev_ptr)
            APS_HIP(hipMemcpy(hp.data(), pair_ptr, (n_pairs + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
        else
            std::copy(pair_ptr, pair_ptr + n_pairs + 1, hp.begin());
        APS_REQUIRE(hp[0] >= 0, APS_E_ARG, "pair_ptr[0] < 0");
        for (int p = 0; p < n_pairs; ++p) APS_REQUIRE(hp[p + 1] >= hp[p], APS_E_ARG, "pair_ptr is not ascending");
        APS_REQUIRE(hp[n_pairs] <= ldu, APS_E_DIM, "pair_ptr[end] = %lld exceeds the leading dimension %lld",
                    (long long)hp[n_pairs], (long long)ldu);
        In<double> dUi(Ui, (size_t)2 * ldu), dUj(Uj, (size_t)2 * ldu), dc(cams, (size_t)n_pairs * 48);
        In<int64_t> dp(pair_ptr, (size_t)n_pairs + 1);
        Out<double> dout(out, (size_t)n_pairs * kBaAcc);
        {
            Prof prof("ba_pair_blocks");
            ba_pair_blocks_kernel<<<(unsigned)n_pairs, 64, 0, stream()>>>(dUi, dUj, ldu, dp, dc, sigma_huber,
                                                                          both_directions ? 1 : 0, dout.get());
        }
        check_launch("ba_pair_blocks_kernel");
        dout.commit();
        APS_HIP(hipStreamSynchronize(stream()));
    });
}

// ---- resident problem -------------------------------------------------------------------------------------------------------

struct aps_ba_problem {
    int device = -1;
    int n_pairs = 0, n_cams = 0;
    int64_t ldu = 0;
    double *Ui = nullptr, *Uj = nullptr;  // 2 x ldu each, as given
    int64_t* ptr = nullptr;               // n_pairs + 1
    int* ij = nullptr;                    // 2 x n_pairs
    int* cam_ptr = nullptr;               // n_cams + 1: camera k's pairs are cam_list[cam_ptr[k] .. cam_ptr[k+1])
    int* cam_list = nullptr;              // 2 x n_pairs entries (pair << 1 | role), role 1 when k is the pair's j; pair order
    int* pair_of = nullptr;               // n_cams x n_cams: the pair of (i, j), i < j, or -1
    double* blocks = nullptr;             // n_pairs x 59
    double* hblocks = nullptr;            // n_pairs x kBaHRec, allocated by the first aps_ba_h_normal_eqns
    // per-evaluation buffers, grown on demand: the inputs (cams base | cams lin | col_start | n_params | row_cam) and the
    // outputs (E r2sum rcnt | g | H), each with a pinned host twin so that one copy moves each way
    void* d_in = nullptr;
    void* h_in = nullptr;
    size_t in_cap = 0;
    double* d_out = nullptr;
    double* h_out = nullptr;
    size_t out_cap = 0;
    std::vector<int> h_ij;
};

namespace {

void ba_problem_free(aps_ba_problem* h) {
    for (void* p : {(void*)h->Ui, (void*)h->Uj, (void*)h->ptr, (void*)h->ij, (void*)h->cam_ptr, (void*)h->cam_list,
                    (void*)h->pair_of, (void*)h->blocks, (void*)h->hblocks, h->d_in, (void*)h->d_out})
        if (p) (void)hipFree(p);
    if (h->h_in) (void)hipHostFree(h->h_in);
    if (h->h_out) (void)hipHostFree(h->h_out);
    delete h;
}

template <class T>
T* dev_upload(const T* src, size_t count) {
    T* d = nullptr;
    APS_HIP(hipMalloc(&d, (count ? count : 1) * sizeof(T)));
    if (count) APS_HIP(hipMemcpyAsync(d, src, count * sizeof(T), hipMemcpyHostToDevice, stream()));
    return d;
}

void require_host(const void* p, const char* what) {
    APS_REQUIRE(!is_device_ptr(p), APS_E_ARG, "%s must be host memory", what);
}

// a device buffer and its pinned host twin of at least `bytes`, regrown (contents dropped) when too small
template <class T>
void ensure_pair(T*& d, T*& host, size_t& cap, size_t bytes) {
    if (bytes <= cap) return;
    if (d) (void)hipFree(d);
    if (host) (void)hipHostFree(host);
    d = host = nullptr;
    cap = 0;
    APS_HIP(hipMalloc((void**)&d, bytes));
    APS_HIP(hipHostMalloc((void**)&host, bytes, hipHostMallocDefault));
    cap = bytes;
}

}  // namespace

extern "C" int aps_ba_problem_create(const double* Ui, const double* Uj, int64_t ldu, const int64_t* pair_ptr,
                                     const int* pair_ij, int n_pairs, int n_cams, aps_ba_problem** handle) {
    return guarded([&] {
        APS_REQUIRE(handle, APS_E_ARG, "NULL handle pointer");
        *handle = nullptr;
        APS_REQUIRE(n_pairs >= 0, APS_E_ARG, "negative pair count");
        APS_REQUIRE(n_cams >= 1, APS_E_ARG, "n_cams must be positive");
        APS_REQUIRE(pair_ptr && (n_pairs == 0 || pair_ij), APS_E_ARG, "NULL argument");
        require_host(pair_ptr, "pair_ptr");
        require_host(pair_ij, "pair_ij");
        APS_REQUIRE(pair_ptr[0] >= 0, APS_E_ARG, "pair_ptr[0] < 0");
        for (int p = 0; p < n_pairs; ++p) {
            APS_REQUIRE(pair_ptr[p + 1] >= pair_ptr[p], APS_E_ARG, "pair_ptr is not ascending");
            const int i = pair_ij[2 * p], j = pair_ij[2 * p + 1];
            APS_REQUIRE(0 <= i && i < j && j < n_cams, APS_E_ARG, "pair %d: need 0 <= i < j < n_cams, got (%d, %d)", p, i, j);
            if (p) {
                const int pi = pair_ij[2 * p - 2], pj = pair_ij[2 * p - 1];
                APS_REQUIRE(pi < i || (pi == i && pj < j), APS_E_ARG, "pairs must be sorted by (i, j) without repeats");
            }
        }
        const int64_t total = pair_ptr[n_pairs];
        APS_REQUIRE(total <= ldu, APS_E_DIM, "pair_ptr[end] = %lld exceeds the leading dimension %lld", (long long)total,
                    (long long)ldu);
        APS_REQUIRE(total == 0 || (Ui && Uj), APS_E_ARG, "NULL argument");
        if (total) {
            require_host(Ui, "Ui");
            require_host(Uj, "Uj");
        }
        ctx();
        std::vector<int> cnt(n_cams + 1, 0), cam_ptr(n_cams + 1, 0), cam_list(2 * (size_t)n_pairs),
            pair_of((size_t)n_cams * n_cams, -1);
        for (int p = 0; p < n_pairs; ++p) {
            ++cnt[pair_ij[2 * p]];
            ++cnt[pair_ij[2 * p + 1]];
            pair_of[(size_t)pair_ij[2 * p] * n_cams + pair_ij[2 * p + 1]] = p;
        }
        for (int k = 0; k < n_cams; ++k) cam_ptr[k + 1] = cam_ptr[k] + cnt[k];
        std::vector<int> fill(cam_ptr.begin(), cam_ptr.end() - 1);
        for (int p = 0; p < n_pairs; ++p) {  // pair order; per camera: first as j (i < k), then as i (j > k)
            cam_list[fill[pair_ij[2 * p]]++] = p << 1;
            cam_list[fill[pair_ij[2 * p + 1]]++] = (p << 1) | 1;
        }
        auto* h = new aps_ba_problem;
        try {
            h->device = ctx().device;
            h->n_pairs = n_pairs;
            h->n_cams = n_cams;
            h->ldu = ldu;
            h->h_ij.assign(pair_ij, pair_ij + 2 * (size_t)n_pairs);
            h->Ui = dev_upload(Ui, total ? (size_t)2 * ldu : 0);
            h->Uj = dev_upload(Uj, total ? (size_t)2 * ldu : 0);
            h->ptr = dev_upload(pair_ptr, (size_t)n_pairs + 1);
            h->ij = dev_upload(pair_ij, (size_t)2 * n_pairs);
            h->cam_ptr = dev_upload(cam_ptr.data(), cam_ptr.size());
            h->cam_list = dev_upload(cam_list.data(), cam_list.size());
            h->pair_of = dev_upload(pair_of.data(), pair_of.size());
            APS_HIP(hipMalloc(&h->blocks, ((size_t)n_pairs * kBaAcc + 1) * sizeof(double)));
            APS_HIP(hipStreamSynchronize(stream()));  // the host vectors above go out of scope
        } catch (...) {
            ba_problem_free(h);
            throw;
        }
        *handle = h;
    });
}

extern "C" int aps_ba_problem_destroy(aps_ba_problem* handle) {
    return guarded([&] {
        if (!handle) return;
        (void)hipStreamSynchronize(stream());
        ba_problem_free(handle);
    });
}

extern "C" int aps_ba_normal_eqns(aps_ba_problem* h, const double* base_cams, const double* lin_cams, const int* col_start,
                                  const int* n_params, int P, double sigma_huber, int both_directions, int want_H, double* H,
                                  double* g, double* stats) {
    return guarded([&] {
        APS_REQUIRE(h, APS_E_ARG, "NULL problem handle");
        APS_REQUIRE(base_cams && lin_cams && col_start && n_params && stats, APS_E_ARG, "NULL argument");
        APS_REQUIRE(!want_H || (H && g), APS_E_ARG, "H and g are required when want_H is set");
        APS_REQUIRE(sigma_huber > 0.0 && std::isfinite(sigma_huber), APS_E_ARG, "sigmaHuber must be positive and finite");
        APS_REQUIRE(P >= 1, APS_E_ARG, "P must be positive");
        const int n = h->n_cams;
        APS_REQUIRE(ctx().device == h->device, APS_E_ARG, "the problem lives on device %d, the calling thread uses %d",
                    h->device, ctx().device);
        for (const void* p : {(const void*)base_cams, (const void*)lin_cams, (const void*)col_start, (const void*)n_params})
            require_host(p, "camera / column arrays");
        for (const void* p : {(const void*)H, (const void*)g, (const void*)stats}) require_host(p, "H, g and stats");
        // the column map: every active camera owns n_params[k] (1 or 4) columns from col_start[k], the active cameras
        // tile 0 .. P-1 exactly
        const size_t cam_bytes = (size_t)n * 12 * sizeof(double);
        const size_t in_bytes = 2 * cam_bytes + ((size_t)2 * n + P) * sizeof(int);
        ensure_pair(h->d_in, h->h_in, h->in_cap, in_bytes);
        char* hin = static_cast<char*>(h->h_in);
        int* h_cs = reinterpret_cast<int*>(hin + 2 * cam_bytes);
        int* h_np = h_cs + n;
        int* h_rc = h_np + n;
        std::fill(h_rc, h_rc + P, -1);
        int64_t cover = 0;
        for (int k = 0; k < n; ++k) {
            const int c = col_start[k];
            h_cs[k] = c;
            h_np[k] = n_params[k];
            APS_REQUIRE(c >= -1, APS_E_ARG, "col_start[%d] = %d (use -1 for a camera outside camList)", k, c);
            if (c < 0) continue;
            const int np = n_params[k];
            APS_REQUIRE(np == 1 || np == 4, APS_E_ARG, "n_params[%d] = %d (1 for the seed, 4 otherwise)", k, np);
            APS_REQUIRE((int64_t)c + np <= P, APS_E_ARG, "camera %d's columns %d..%d do not fit P = %d", k, c, c + np - 1, P);
            for (int e = 0; e < np; ++e) {
                APS_REQUIRE(h_rc[c + e] < 0, APS_E_ARG, "col_start overlaps: column %d belongs to cameras %d and %d", c + e,
                            h_rc[c + e], k);
                h_rc[c + e] = k;
            }
            cover += np;
        }
        APS_REQUIRE(cover == P, APS_E_ARG, "P = %d but the column map covers %lld columns", P, (long long)cover);
        std::memcpy(hin, base_cams, cam_bytes);
        std::memcpy(hin + cam_bytes, lin_cams, cam_bytes);
        const size_t out_n = 3 + (want_H ? (size_t)P + (size_t)P * P : 0);
        ensure_pair(h->d_out, h->h_out, h->out_cap, out_n * sizeof(double));
        hipStream_t st = stream();
        APS_HIP(hipMemcpyAsync(h->d_in, h->h_in, in_bytes, hipMemcpyHostToDevice, st));
        const char* din = static_cast<const char*>(h->d_in);
        const double* d_base = reinterpret_cast<const double*>(din);
        const double* d_lin = reinterpret_cast<const double*>(din + cam_bytes);
        const int* d_cs = reinterpret_cast<const int*>(din + 2 * cam_bytes);
        const int both = both_directions ? 1 : 0;
        if (h->n_pairs > 0) {
            Prof prof("ba_normal_blocks");
            if (want_H)
                ba_problem_blocks_kernel<true><<<(unsigned)h->n_pairs, 64, 0, st>>>(h->Ui, h->Uj, h->ldu, h->ptr, h->ij, d_base,
                                                                                  d_lin, d_cs, sigma_huber, both, h->blocks);
            else
                ba_problem_blocks_kernel<false><<<(unsigned)h->n_pairs, 64, 0, st>>>(h->Ui, h->Uj, h->ldu, h->ptr, h->ij, d_base,
                                                                                   d_lin, d_cs, sigma_huber, both, h->blocks);
        }
        check_launch("ba_problem_blocks_kernel");
        {
            Prof prof("ba_normal_assemble");
            ba_assemble_kernel<<<want_H ? (unsigned)n + 1 : 1u, 256, 0, st>>>(h->blocks, h->ij, h->ptr, h->cam_ptr, h->cam_list,
                                                                              h->pair_of, d_cs, d_cs + n, d_cs + 2 * n, n,
                                                                              h->n_pairs, P, h->d_out);
        }
        check_launch("ba_assemble_kernel");
        APS_HIP(hipMemcpyAsync(h->h_out, h->d_out, out_n * sizeof(double), hipMemcpyDeviceToHost, st));
        APS_HIP(hipStreamSynchronize(st));
        const double R2 = h->h_out[1], cnt = h->h_out[2];
        stats[0] = h->h_out[0];
        // rmse = sqrt(max(R2sum, 0) / max(Rcnt, 1)) with the host mirror's max (the first argument unless the second is larger)
        stats[1] = std::sqrt((0.0 > R2 ? 0.0 : R2) / (1.0 > cnt ? 1.0 : cnt));
        if (want_H) {
            std::memcpy(g, h->h_out + 3, (size_t)P * sizeof(double));
            std::memcpy(H, h->h_out + 3 + P, (size_t)P * P * sizeof(double));
        }
    });
}

extern "C" int aps_ba_h_normal_eqns(aps_ba_problem* h, const double* G, int n_cams, int seed, double huber, int want_H,
                                    double* H, double* g, double* stats) {
    return guarded([&] {
        APS_REQUIRE(h, APS_E_ARG, "NULL problem handle");
        APS_REQUIRE(G && stats, APS_E_ARG, "NULL argument");
        APS_REQUIRE(!want_H || (H && g), APS_E_ARG, "H and g are required when want_H is set");
        APS_REQUIRE(n_cams == h->n_cams, APS_E_ARG, "n_cams = %d but the problem has %d images", n_cams, h->n_cams);
        APS_REQUIRE(n_cams >= 2, APS_E_ARG, "the homography adjustment needs at least two images");
        APS_REQUIRE(0 <= seed && seed < n_cams, APS_E_ARG, "seed %d outside 0 .. %d", seed, n_cams - 1);
        APS_REQUIRE(std::isfinite(huber), APS_E_ARG, "Huber must be finite");
        APS_REQUIRE(ctx().device == h->device, APS_E_ARG, "the problem lives on device %d, the calling thread uses %d",
                    h->device, ctx().device);
        require_host(G, "G");
        for (const void* p : {(const void*)H, (const void*)g, (const void*)stats}) require_host(p, "H, g and stats");
        const int n = n_cams;
        for (int k = 0; k < n; ++k) APS_REQUIRE(G[9 * k + 8] == 1.0, APS_E_ARG, "G of image %d has H(3,3) != 1", k);
        const double delta = huber > 0.0 ? huber : 0.0;  // max(0, opts.Huber)
        const int P = 8 * (n - 1);
        // inputs: G (n x 9) | col_start (n) | blk_cam (n - 1)
        const size_t g_bytes = (size_t)n * 9 * sizeof(double);
        const size_t in_bytes = g_bytes + ((size_t)2 * n - 1) * sizeof(int);
        ensure_pair(h->d_in, h->h_in, h->in_cap, in_bytes);
        char* hin = static_cast<char*>(h->h_in);
        std::memcpy(hin, G, g_bytes);
        int* h_cs = reinterpret_cast<int*>(hin + g_bytes);
        int* h_bc = h_cs + n;
        for (int k = 0, blk = 0; k < n; ++k) {
            if (k == seed) {
                h_cs[k] = -1;
                continue;
            }
            h_cs[k] = 8 * blk;
            h_bc[blk++] = k;
        }
        const size_t out_n = 3 + (want_H ? (size_t)P + (size_t)P * P : 0);
        ensure_pair(h->d_out, h->h_out, h->out_cap, out_n * sizeof(double));
        if (!h->hblocks) APS_HIP(hipMalloc(&h->hblocks, ((size_t)h->n_pairs * kBaHRec + 1) * sizeof(double)));
        hipStream_t st = stream();
        APS_HIP(hipMemcpyAsync(h->d_in, h->h_in, in_bytes, hipMemcpyHostToDevice, st));
        const char* din = static_cast<const char*>(h->d_in);
        const double* d_G = reinterpret_cast<const double*>(din);
        const int* d_cs = reinterpret_cast<const int*>(din + g_bytes);
        if (h->n_pairs > 0) {
            Prof prof("ba_h_blocks");
            if (want_H)
                ba_h_blocks_kernel<true><<<dim3((unsigned)h->n_pairs, 3), 64, 0, st>>>(h->Ui, h->Uj, h->ldu, h->ptr, h->ij, d_G,
                                                                                     delta, h->hblocks);
            else
                ba_h_blocks_kernel<false><<<dim3((unsigned)h->n_pairs, 1), 64, 0, st>>>(h->Ui, h->Uj, h->ldu, h->ptr, h->ij,
                                                                                      d_G, delta, h->hblocks);
        }
        check_launch("ba_h_blocks_kernel");
        {
            Prof prof("ba_h_assemble");
            ba_h_assemble_kernel<<<want_H ? (unsigned)n + 1 : 1u, 256, 0, st>>>(h->hblocks, h->ij, h->ptr, h->cam_ptr,
                                                                                h->cam_list, h->pair_of, d_cs, d_cs + n, n,
                                                                                h->n_pairs, P, h->d_out);
        }
        check_launch("ba_h_assemble_kernel");
        APS_HIP(hipMemcpyAsync(h->h_out, h->d_out, out_n * sizeof(double), hipMemcpyDeviceToHost, st));
        APS_HIP(hipStreamSynchronize(st));
        std::memcpy(stats, h->h_out, 3 * sizeof(double));
        if (want_H) {
            std::memcpy(g, h->h_out + 3, (size_t)P * sizeof(double));
            std::memcpy(H, h->h_out + 3 + P, (size_t)P * P * sizeof(double));
        }
    });
}
