// kernels_vialign.h — visual-inertial alignment (lfvio_vi_align, include/lfvio.h): VisualIMUAlignment of
// initial/initial_aligment.cpp:3-216 on the device, between two launches of k_preintegrate.
//   k_va_bias    solveGyroscopeBias (:3-36): the 3 x 3 normal equations over the F - 1 consecutive pairs, delta_bg, and the new
//                bias written into the ImuJobs where they lie (ba = 0, bg = Bgs[0] + delta_bg: repropagate of :34)
//   k_va_align   LinearAlignment (:121-206) and the four iterations of RefineGravity (:53-119), five dependent solves in one launch
// Both are one workgroup: a latency problem (F <= 128 pairs of a few hundred flops each), not a throughput one.
//
// The normal matrix is an arrowhead: 3 x 3 velocity blocks D_f on the diagonal, E_f = A[3f : 3f + 3, 3f + 3 : 3f + 6] beside it
// (pair f couples frames f and f + 1 only), a dense border B of M columns (M = 4: gravity and scale; M = 3: the two tangent
// coordinates and scale) and the M x M corner C.  Thread f builds pair f, hands the part that falls on frame f + 1 over through
// LDS, and frame f's owner adds the two overlapping contributions in pair order (:102, :167) — fixed order, no atomics.  The
// corner sums are taken over the pairs in order by one thread per entry.  RefineGravity zeroes A and b ONCE, in front of its loop
// (:61-64), and scales them by 1000 inside it (:111-112): iteration k solves 1000 (A_{k-1} + S_k).  The accumulators A_{k-1}
// therefore live in the registers of the threads that own them for the whole launch; LDS holds the working copy that the
// factorization destroys.
//
// Factorization: block elimination along the chain without pivoting (Eigen's ldlt() pivots; a pivot that is not > 0 ends the
// call with status 3).  Lane c < 3 + M + 1 of wave 0 carries column c of [D'_f | B'_f | b'_f]; per frame the six entries of D'_f
// are broadcast (v_readlane), every lane factors the same 3 x 3 LDL^T and solves its own column: W = D'^-1 [E_f | B'_f | b'_f],
// then [D' | B' | b']_{f + 1} = [D | B | b]_{f + 1} - E_f^T W.  The corner's Schur sums B'^T W are formed per frame in parallel and
// added in frame order, the corner is solved by one thread, and x_f = w_b - W_B x_c - W_E x_{f + 1} runs back along the chain.
// The forward chain (F dependent 3 x 3 factorizations) bounds the kernel.
//
// LDS: 53 doubles per frame (54 KB at F = 128) + the solution; a dense n x n (n up to 388: 1.2 MB) is never formed.
#pragma once
#include "dev_math.h"
#include "dev_types.h"
#include "kernels_feat.h"

constexpr int VA_MAX_FRAMES = LFVIO_MAX_IMAGE_FRAMES, VA_THREADS = 128;
static_assert(VA_THREADS >= VA_MAX_FRAMES, "one thread per image frame");

struct VaParams {
  double tic[3], g_norm;
};

// LDL^T of a symmetric 3 x 3 (lower triangle a00 a10 a20 a11 a21 a22) without pivoting; id* = 1 / d*
struct ldl3 {
  double l10, l20, l21, id0, id1, id2;
  bool ok;
};
DEV ldl3 ldl3_factor(double a00, double a10, double a20, double a11, double a21, double a22) {
  ldl3 f;
  f.id0 = 1.0 / a00;
  f.l10 = a10 * f.id0, f.l20 = a20 * f.id0;
  const double d1 = a11 - f.l10 * a10;
  f.id1 = 1.0 / d1;
  f.l21 = (a21 - f.l20 * a10) * f.id1;
  const double d2 = a22 - f.l20 * a20 - f.l21 * (f.l21 * d1);
  f.id2 = 1.0 / d2;
  f.ok = a00 > 0.0 && d1 > 0.0 && d2 > 0.0;
  return f;
}
DEV d3 ldl3_solve(const ldl3 &f, d3 r) {
  const double y1 = r.y - f.l10 * r.x, y2 = r.z - f.l20 * r.x - f.l21 * y1;
  d3 x;
  x.z = y2 * f.id2;
  x.y = y1 * f.id1 - f.l21 * x.z;
  x.x = r.x * f.id0 - f.l10 * x.y - f.l20 * x.z;
  return x;
}
// Eigen's normalized(): v / sqrt(squaredNorm), a zero vector returned as it is (TangentBasis of g along -z, :45).  A division, not a
// reciprocal: (0, 0, c) must come out as (0, 0, 1) exactly for the comparison of :43
DEV d3 normalized3(d3 v) {
  const double n2 = v.x * v.x + v.y * v.y + v.z * v.z;
  if (!(n2 > 0.0)) return v;
  const double n = sqrt(n2);
  return mk3(v.x / n, v.y / n, v.z / n);
}
DEV double norm3(d3 v) { return sqrt(v.x * v.x + v.y * v.y + v.z * v.z); }

// ---- solveGyroscopeBias: one workgroup, thread i = pair (i, i + 1); pre[i] is the pre-integration of span i + 1
__global__ __launch_bounds__(VA_THREADS) void k_va_bias(int F, const double *R, const LfvioPreintegration *pre, ImuJob *jobs,
                                                       LfvioViAlignOut *out) {
  __shared__ double part[VA_MAX_FRAMES][12], sum[12], sol[4];
  const int i = threadIdx.x;
  if (i < F - 1) {
    const m33 Ri = ldm(R + 9 * i), Rj = ldm(R + 9 * (i + 1));
    const q4 q_ij = R2q(mm(tr(Ri), Rj));  // :19
    const LfvioPreintegration *p = &pre[i];
    m33 J;  // jacobian.block<3, 3>(O_R, O_BG), :20
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
      for (int c = 0; c < 3; c++) J.a[3 * r + c] = p->jacobian[(3 + r) * 15 + 12 + c];
    const q4 dq = q4{p->delta_q[3], p->delta_q[0], p->delta_q[1], p->delta_q[2]};
    const d3 tb = 2.0 * qvec(qmul(qinv(dq), q_ij));  // :21
    const m33 JtJ = mm(tr(J), J);
    const d3 Jtb = vmul(tb, J);
#pragma unroll
    for (int e = 0; e < 9; e++) part[i][e] = JtJ.a[e];
    part[i][9] = Jtb.x, part[i][10] = Jtb.y, part[i][11] = Jtb.z;
  }
  const d3 bg0 = ld3(jobs[0].bg);  // Bgs[0]: span[1].linearized_bg as passed
  __syncthreads();
  if (i < 12) {  // :22-23, in pair order
    double s = 0.0;
    for (int k = 0; k < F - 1; k++) s += part[k][i];
    sum[i] = s;
  }
  __syncthreads();
  if (i == 0) {
    const ldl3 f = ldl3_factor(sum[0], sum[3], sum[6], sum[4], sum[7], sum[8]);
    const d3 x = ldl3_solve(f, mk3(sum[9], sum[10], sum[11]));  // :25
    sol[0] = x.x, sol[1] = x.y, sol[2] = x.z, sol[3] = f.ok ? 1.0 : 0.0;
  }
  __syncthreads();
  if (sol[3] == 0.0) {  // the jobs keep their biases; k_va_align sees the status and leaves
    if (i == 0) out->status = 3;
    return;
  }
  if (i < F - 1) {  // :28-34: ba = 0, bg = Bgs[0] + delta_bg for the second launch of k_preintegrate
#pragma unroll
    for (int k = 0; k < 3; k++) jobs[i].ba[k] = 0.0, jobs[i].bg[k] = (k == 0 ? bg0.x : k == 1 ? bg0.y : bg0.z) + sol[k];
  }
  if (i == 0) out->status = 0, out->delta_bg[0] = sol[0], out->delta_bg[1] = sol[1], out->delta_bg[2] = sol[2];
}

// ---- the arrowhead system in LDS: per frame D (3 x 3), E (3 x 3), B (3 x 4, M columns used), b (3), and a 20-double slot for
// what is summed over frames (the pairs' corner blocks, then the Schur sums) and, in between, W_B | w_b
struct VaSys {
  double D[VA_MAX_FRAMES][9], E[VA_MAX_FRAMES][9], B[VA_MAX_FRAMES][12], b[VA_MAX_FRAMES][3], S[VA_MAX_FRAMES][20];
  double C[20];   // corner: M x M row-major, then its right-hand side
  double xc[4];   // border solution
  double x[3 * VA_MAX_FRAMES];
  double L[9];    // border basis: column k of the identity (LinearAlignment) or of TangentBasis (RefineGravity)
  double g0[3];
  int bad;
};

// What pair f does not change between the five solves
struct VaPair {
  m33 RiT, Rij;
  d3 h, b0, dv;  // R_i^T (T_j - T_i) / 100; delta_p + R_ij tic - tic; delta_v
  double dt;
};

// One set of blocks (:73-110, :134-175) added to the accumulators, the sum scaled by 1000 (:111-112, :176-177) and copied into
// the working system.  M - 1 gravity columns L (sys.L) and the scale column; g0 enters the right-hand side when REFINE.
template <int M, bool REFINE>
DEV void va_build(VaSys &sys, int F, int f, const VaPair &p, double (&aD)[9], double (&aE)[9], double (&aB)[12], double (&ab)[3],
                  double &aC) {
  constexpr int K = M - 1;
  double iD = 0.0, iB[3][M], ib[3];
  m33 E;
#pragma unroll
  for (int e = 0; e < 9; e++) E.a[e] = 0.0;
#pragma unroll
  for (int r = 0; r < 3; r++) {
    ib[r] = 0.0;
#pragma unroll
    for (int k = 0; k < M; k++) iB[r][k] = 0.0;
  }
  if (f < F - 1) {
    const double dt = p.dt, h2 = dt * dt / 2;
    d3 U[M], V[M];  // columns 6.. of the two row blocks of tmp_A
#pragma unroll
    for (int k = 0; k < K; k++) {
      const d3 rl = mul(p.RiT, mk3(sys.L[k], sys.L[3 + k], sys.L[6 + k]));
      U[k] = rl * h2, V[k] = rl * dt;  // :85, :91, :146, :152
    }
    U[K] = p.h, V[K] = mk3(0, 0, 0);  // :86, :147
    d3 b0 = p.b0, b1 = p.dv;          // :87, :92, :148, :153
    if (REFINE) {
      const d3 rg = mul(p.RiT, ld3(sys.g0));
      b0 = b0 - rg * h2, b1 = b1 - rg * dt;
    }
    // r_A = tmp_A^T tmp_A, r_b = tmp_A^T tmp_b with tmp_A = [-dt I, 0, U; -I, R_ij, V]
    iD = dt * dt + 1.0;
    const m33 RtR = mm(tr(p.Rij), p.Rij);
#pragma unroll
    for (int e = 0; e < 9; e++) E.a[e] = -p.Rij.a[e], sys.D[f + 1][e] = RtR.a[e];
    const d3 bt = -(b0 * dt) - b1, bm = vmul(b1, p.Rij);
    ib[0] = bt.x, ib[1] = bt.y, ib[2] = bt.z;
    sys.b[f + 1][0] = bm.x, sys.b[f + 1][1] = bm.y, sys.b[f + 1][2] = bm.z;
#pragma unroll
    for (int k = 0; k < M; k++) {
      const d3 t = -(U[k] * dt) - V[k], m = vmul(V[k], p.Rij);
      iB[0][k] = t.x, iB[1][k] = t.y, iB[2][k] = t.z;
      sys.B[f + 1][k] = m.x, sys.B[f + 1][4 + k] = m.y, sys.B[f + 1][8 + k] = m.z;
#pragma unroll
      for (int l = 0; l < M; l++) sys.S[f][M * k + l] = dot(U[k], U[l]) + dot(V[k], V[l]);
      sys.S[f][M * M + k] = dot(U[k], b0) + dot(V[k], b1);
    }
  }
  __syncthreads();
  if (f < F) {  // frame f: what pair f - 1 left here, then pair f (:102-109, :167-174)
#pragma unroll
    for (int e = 0; e < 9; e++) {
      const double j = f > 0 ? sys.D[f][e] : 0.0;
      aD[e] = ((aD[e] + j) + (e % 4 == 0 ? iD : 0.0)) * 1000.0;
      aE[e] = (aE[e] + E.a[e]) * 1000.0;
      sys.D[f][e] = aD[e], sys.E[f][e] = aE[e];
    }
#pragma unroll
    for (int r = 0; r < 3; r++) {
      const double j = f > 0 ? sys.b[f][r] : 0.0;
      ab[r] = ((ab[r] + j) + ib[r]) * 1000.0;
      sys.b[f][r] = ab[r];
#pragma unroll
      for (int k = 0; k < M; k++) {
        const double jb = f > 0 ? sys.B[f][4 * r + k] : 0.0;
        aB[4 * r + k] = ((aB[4 * r + k] + jb) + iB[r][k]) * 1000.0;
        sys.B[f][4 * r + k] = aB[4 * r + k];
      }
    }
  }
  if (f < M * M + M) {  // the corner and its right-hand side over the pairs in order (:105-106, :170-171)
    double s = aC;
    for (int k = 0; k < F - 1; k++) s += sys.S[k][f];
    aC = s * 1000.0;
    sys.C[f] = aC;
  }
  __syncthreads();
}

// Solve the working system; x -> sys.x (3F velocities), sys.xc (border).  Ends with a barrier; sys.bad != 0: a pivot was not > 0.
template <int M>
DEV void va_solve(VaSys &sys, int F, int tid) {
  constexpr int NC = 3 + M + 1;  // columns of [D | B | b]
  if (tid < 64) {
    const int c = tid & 7;
    auto col = [&](int f) {
      if (c < 3) return mk3(sys.D[f][c], sys.D[f][3 + c], sys.D[f][6 + c]);
      if (c < 3 + M) return mk3(sys.B[f][c - 3], sys.B[f][4 + c - 3], sys.B[f][8 + c - 3]);
      if (c == 3 + M) return ld3(sys.b[f]);
      return mk3(0, 0, 0);
    };
    d3 m = col(0);
    for (int f = 0; f < F; f++) {
      const ldl3 fc = ldl3_factor(readlane_f64(m.x, 0), readlane_f64(m.y, 0), readlane_f64(m.z, 0), readlane_f64(m.y, 1),
                                  readlane_f64(m.z, 1), readlane_f64(m.z, 2));
      if (!fc.ok) {
        if (tid == 0) sys.bad = 1;
        break;
      }
      const m33 E = ldm(sys.E[f]);  // zero for the last frame
      const int ce = c < 3 ? c : 0;  // (the column comes from LDS: a run-time index into E would put it in scratch memory)
      const d3 w = ldl3_solve(fc, c < 3 ? mk3(sys.E[f][ce], sys.E[f][3 + ce], sys.E[f][6 + ce]) : m);
      if (tid < 3) {
        sys.E[f][c] = w.x, sys.E[f][3 + c] = w.y, sys.E[f][6 + c] = w.z;  // W_E
      } else if (tid < NC) {
        double *s = &sys.S[f][3 * (c - 3)];
        s[0] = w.x, s[1] = w.y, s[2] = w.z;  // W_B | w_b
        if (c < 3 + M) sys.B[f][c - 3] = m.x, sys.B[f][4 + c - 3] = m.y, sys.B[f][8 + c - 3] = m.z;  // B'
        else sys.b[f][0] = m.x, sys.b[f][1] = m.y, sys.b[f][2] = m.z;                                  // b'
      }
      if (f + 1 < F) m = col(f + 1) - vmul(w, E);
    }
  }
  __syncthreads();
  if (sys.bad) return;
  // Schur sums of the corner: frame f's B'^T [W_B | w_b]
  double W[3 * (M + 1)];
  if (tid < F) {
#pragma unroll
    for (int e = 0; e < 3 * (M + 1); e++) W[e] = sys.S[tid][e];
#pragma unroll
    for (int k = 0; k < M; k++) {
      const d3 bk = mk3(sys.B[tid][k], sys.B[tid][4 + k], sys.B[tid][8 + k]);
#pragma unroll
      for (int l = 0; l < M; l++) sys.S[tid][M * k + l] = dot(bk, mk3(W[3 * l], W[3 * l + 1], W[3 * l + 2]));
      sys.S[tid][M * M + k] = dot(bk, mk3(W[3 * M], W[3 * M + 1], W[3 * M + 2]));
    }
  }
  __syncthreads();
  if (tid < M * M + M) {
    double s = sys.C[tid];
    for (int f = 0; f < F; f++) s -= sys.S[f][tid];
    sys.C[tid] = s;
  }
  __syncthreads();
  if (tid == 0) {  // M x M LDL^T without pivoting
    double a[M][M], d[M], y[M];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < M; j++) {
      double dj = sys.C[M * j + j];
#pragma unroll
      for (int k = 0; k < j; k++) dj -= a[j][k] * a[j][k] * d[k];
      d[j] = dj, ok = ok && dj > 0.0;
#pragma unroll
      for (int i = j + 1; i < M; i++) {
        double v = sys.C[M * i + j];
#pragma unroll
        for (int k = 0; k < j; k++) v -= a[i][k] * a[j][k] * d[k];
        a[i][j] = v / dj;
      }
    }
#pragma unroll
    for (int i = 0; i < M; i++) {
      double v = sys.C[M * M + i];
#pragma unroll
      for (int k = 0; k < i; k++) v -= a[i][k] * y[k];
      y[i] = v;
    }
#pragma unroll
    for (int i = M - 1; i >= 0; i--) {
      double v = y[i] / d[i];
#pragma unroll
      for (int k = i + 1; k < M; k++) v -= a[k][i] * y[k];
      y[i] = v;
    }
#pragma unroll
    for (int i = 0; i < M; i++) sys.xc[i] = y[i];
    if (!ok) sys.bad = 1;
  }
  __syncthreads();
  if (sys.bad) return;
  if (tid < F) {  // w_b - W_B x_c
#pragma unroll
    for (int r = 0; r < 3; r++) {
      double v = W[3 * M + r];
#pragma unroll
      for (int k = 0; k < M; k++) v -= W[3 * k + r] * sys.xc[k];
      sys.b[tid][r] = v;
    }
  }
  __syncthreads();
  if (tid < 64) {  // x_f = t_f - W_E x_{f + 1}, lane r = row r
    const int r = tid < 3 ? tid : 0;
    double x = 0.0;
    for (int f = F - 1; f >= 0; f--) {
      const double x0 = readlane_f64(x, 0), x1 = readlane_f64(x, 1), x2 = readlane_f64(x, 2);
      x = sys.b[f][r] - (sys.E[f][3 * r] * x0 + sys.E[f][3 * r + 1] * x1 + sys.E[f][3 * r + 2] * x2);
      if (tid < 3) sys.x[3 * f + r] = x;
    }
  }
  __syncthreads();
}

// TangentBasis (:38-51) of g0 into sys.L (3 x 2 in the first two columns)
DEV void va_tangent_basis(VaSys &sys, d3 g0) {
  const d3 a = normalized3(g0);
  d3 tmp = mk3(0, 0, 1);
  if (a.x == tmp.x && a.y == tmp.y && a.z == tmp.z) tmp = mk3(1, 0, 0);  // :43, the exact comparison
  const d3 b = normalized3(tmp - a * dot(a, tmp)), c = cross(a, b);
  sys.L[0] = b.x, sys.L[3] = b.y, sys.L[6] = b.z;
  sys.L[1] = c.x, sys.L[4] = c.y, sys.L[7] = c.z;
}

// ---- LinearAlignment + RefineGravity: one workgroup, thread f = frame f and pair (f, f + 1)
__global__ __launch_bounds__(VA_THREADS) void k_va_align(int F, const double *R, const double *T, const LfvioPreintegration *pre,
                                                        const VaParams *prm, LfvioViAlignOut *out, double *x) {
  __shared__ VaSys sys;
  const int f = threadIdx.x;
  if (out->status != 0) return;  // k_va_bias met a pivot that is not > 0
  const double G = prm->g_norm;
  VaPair p;
  if (f < F - 1) {
    const m33 Rj = ldm(R + 9 * (f + 1));
    const d3 tic = ld3(prm->tic);
    p.RiT = tr(ldm(R + 9 * f));
    p.Rij = mm(p.RiT, Rj);
    const d3 h = mul(p.RiT, ld3(T + 3 * (f + 1)) - ld3(T + 3 * f));
    p.h = mk3(h.x / 100.0, h.y / 100.0, h.z / 100.0);
    p.b0 = ld3(pre[f].delta_p) + mul(p.Rij, tic) - tic;
    p.dv = ld3(pre[f].delta_v);
    p.dt = pre[f].sum_dt;
  }
  if (f < 9) sys.L[f] = f % 4 == 0 ? 1.0 : 0.0;
  if (f == 0) sys.bad = 0;
  if (f < F) {
#pragma unroll
    for (int e = 0; e < 9; e++) sys.E[f][e] = 0.0;
  }
  __syncthreads();
  double aD[9], aE[9], aB[12], ab[3], aC = 0.0;
  auto clear = [&]() {
#pragma unroll
    for (int e = 0; e < 9; e++) aD[e] = 0.0, aE[e] = 0.0;
#pragma unroll
    for (int e = 0; e < 12; e++) aB[e] = 0.0;
    ab[0] = ab[1] = ab[2] = 0.0;
    aC = 0.0;
  };
  // ---- LinearAlignment
  clear();
  va_build<4, false>(sys, F, f, p, aD, aE, aB, ab, aC);
  va_solve<4>(sys, F, f);
  if (sys.bad) {
    if (f == 0) out->status = 3;
    return;
  }
  const d3 gl = ld3(sys.xc);
  const double sl = sys.xc[3] / 100.0;  // :179
  if (f == 0) out->g_linear[0] = gl.x, out->g_linear[1] = gl.y, out->g_linear[2] = gl.z, out->s_linear = sl;
  if (fabs(norm3(gl) - G) > 1.0 || sl < 0) {  // :186
    if (f == 0) out->status = 1;
    return;
  }
  // ---- RefineGravity: A and b zeroed once (:61-64)
  clear();
  d3 g0 = normalized3(gl) * G;  // :55
#pragma unroll 1
  for (int k = 0; k < 4; k++) {
    if (f == 0) {
      va_tangent_basis(sys, g0);
      sys.g0[0] = g0.x, sys.g0[1] = g0.y, sys.g0[2] = g0.z;
    }
    __syncthreads();
    va_build<3, true>(sys, F, f, p, aD, aE, aB, ab, aC);
    va_solve<3>(sys, F, f);
    if (sys.bad) {
      if (f == 0) out->status = 3;
      return;
    }
    const d3 lx = mk3(sys.L[0], sys.L[3], sys.L[6]), ly = mk3(sys.L[1], sys.L[4], sys.L[7]);
    g0 = normalized3(g0 + lx * sys.xc[0] + ly * sys.xc[1]) * G;  // :115
    if (f == 0) out->g_iter[k][0] = g0.x, out->g_iter[k][1] = g0.y, out->g_iter[k][2] = g0.z;
    __syncthreads();  // everybody has read the basis before thread 0 writes the next one
  }
  const double s = sys.xc[2] / 100.0;  // :197
  if (f == 0) {
    out->g[0] = g0.x, out->g[1] = g0.y, out->g[2] = g0.z, out->s = s;
    out->status = s < 0.0 ? 2 : 0;  // :201
  }
  for (int e = f; e < 3 * F; e += VA_THREADS) x[e] = sys.x[e];
}
