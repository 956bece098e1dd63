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
                    (void*)h->pair_of, (void*)h->blocks, h->d_in, (void*)h->d_out})
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
        if (in_bytes > h->in_cap) {
            if (h->d_in) (void)hipFree(h->d_in);
            if (h->h_in) (void)hipHostFree(h->h_in);
            h->d_in = h->h_in = nullptr;
            h->in_cap = 0;
            APS_HIP(hipMalloc(&h->d_in, in_bytes));
            APS_HIP(hipHostMalloc(&h->h_in, in_bytes, hipHostMallocDefault));
            h->in_cap = in_bytes;
        }
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
        if (out_n > h->out_cap) {
            if (h->d_out) (void)hipFree(h->d_out);
            if (h->h_out) (void)hipHostFree(h->h_out);
            h->d_out = h->h_out = nullptr;
            h->out_cap = 0;
            APS_HIP(hipMalloc(&h->d_out, out_n * sizeof(double)));
            APS_HIP(hipHostMalloc(&h->h_out, out_n * sizeof(double), hipHostMallocDefault));
            h->out_cap = out_n;
        }
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
