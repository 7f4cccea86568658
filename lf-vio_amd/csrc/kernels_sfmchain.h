// kernels_sfmchain.h — the incremental part of GlobalSFM::construct (vins_estimator/src/initial/initial_sfm.cpp:121-218): from the relative
// pose of frames l and F - 1 to a pose per keyframe and a position per point, the inputs of the bundle adjustment (kernels_sfmba.h).
//
//   k_sfm_chain : ONE workgroup of 256 threads runs the whole schedule; every step needs the one before it
//     schedule       thread 0 writes the op table: {PnP i, triangulate (i, F - 1)} forward (:157-175), triangulate (l, i) (:177-178),
//                    {PnP i, triangulate (i, l)} backward (:181-195), the closing loop (:197-218) — at most 3 F - 4 ops
//     poses l, F-1   thread 0: Quaterniond(relative_R), inverse(), toRotationMatrix() (:125-153), dev_math.h's Eigen forms
//     PnP op         solveFrameByPnP (:23-71): the points with state == true seen in frame i, in ascending j — a contiguous block of
//                    points per thread, a block prefix scan of the counts, (point, bearing) pairs written in order; then pnp_pose
//                    (kernels_pnp.h), the one call site of the loop
//     triangulation  triangulateTwoFrames (:73-110) / the closing loop: a thread per point with state == false; the 4 x 4 design
//                    matrix (:9-14), jacobi_cols<4, 4>, the column of smallest squared norm divided by its fourth entry (:16-20)
//
// state == true is tri_op[j] >= 0; a position is written once and never changes.  No atomics, a fixed order everywhere: a repeated
// call returns the same bits.  Every loop is bounded by a size (the op count, P, P / 256, F).
#pragma once
#include "kernels_pnp.h"
#include "../../include/lfvio.h"

constexpr int SFMCH_THREADS = PNP_THREADS, SFMCH_MAX_POINTS = 4096, SFMCH_MAX_OPS = 3 * LFVIO_NUM_FRAMES - 4, SFMCH_MIN_PNP = 10;
constexpr int SFMCH_PNP = 0, SFMCH_TRI = 1, SFMCH_CLOSE = 2;

struct SfmChainHead {
  int F, l, P, pad;
  double relative_R[9], relative_T[3];
};
struct SfmChainResult {
  LfvioSfmConstructOut o;
  int posed[LFVIO_NUM_FRAMES], pad;  // frames whose rows of c_rotation, c_translation the chain wrote
};

// triangulatePoint (:6-21) on two 3 x 4 poses (row-major) and two bearings.  A zero fourth entry gives inf / NaN, as there.
DEV d3 sfmch_triangulate(const double *P0, const double *P1, d3 u0, d3 u1) {
  double B[4][4], V[4][4], n2[4];
#pragma unroll
  for (int c = 0; c < 4; c++) {
    B[0][c] = u0.x * P0[8 + c] - u0.z * P0[c];
    B[1][c] = u0.y * P0[8 + c] - u0.z * P0[4 + c];
    B[2][c] = u1.x * P1[8 + c] - u1.z * P1[c];
    B[3][c] = u1.y * P1[8 + c] - u1.z * P1[4 + c];
  }
  jacobi_cols<4, 4>(B, V, 2.3e-16);
#pragma unroll
  for (int c = 0; c < 4; c++) n2[c] = B[0][c] * B[0][c] + B[1][c] * B[1][c] + B[2][c] * B[2][c] + B[3][c] * B[3][c];
  double bn = n2[0], v[4] = {V[0][0], V[1][0], V[2][0], V[3][0]};
#pragma unroll
  for (int c = 1; c < 4; c++) {  // (compare-exchange: a computed column index would put V in scratch memory)
    const bool take = n2[c] < bn;
    bn = take ? n2[c] : bn;
#pragma unroll
    for (int r = 0; r < 4; r++) v[r] = take ? V[r][c] : v[r];
  }
  return mk3(v[0] / v[3], v[1] / v[3], v[2] / v[3]);
}

// gpw, gus [P][3] and gal [P][4]: the gathered correspondences of the PnP in hand and their barycentric coordinates (device memory).
__global__ __launch_bounds__(SFMCH_THREADS) void k_sfm_chain(const SfmChainHead *hd, const int *off, const int *frm, const int *slot, const double *bearing,
                                                              double *qo, double *to, double *X, int *tri_op, double *gpw, double *gus, double *gal,
                                                              SfmChainResult *res) {
  constexpr int NT = SFMCH_THREADS, NF = LFVIO_NUM_FRAMES;
  __shared__ double red[40 * NT / 64], ut[4][12], sbeta[3][4], s_pose[NF][12];
  __shared__ int s_kind[SFMCH_MAX_OPS], s_a[SFMCH_MAX_OPS], s_b[SFMCH_MAX_OPS], s_nops, s_flag, s_scan[NT];
  const int tid = threadIdx.x, F = hd->F, l = hd->l, P = hd->P;

  if (tid == 0) {
    int n = 0;
    auto push = [&](int kind, int a, int b) {
      if (n < SFMCH_MAX_OPS) s_kind[n] = kind, s_a[n] = a, s_b[n] = b, n++;
    };
    for (int i = l; i < F - 1; i++) {  // :157-175
      if (i > l) push(SFMCH_PNP, i, i);
      push(SFMCH_TRI, i, F - 1);
    }
    for (int i = l + 1; i < F - 1; i++) push(SFMCH_TRI, l, i);  // :177-178
    for (int i = l - 1; i >= 0; i--) push(SFMCH_PNP, i, i), push(SFMCH_TRI, i, l);  // :181-195
    push(SFMCH_CLOSE, 0, 0);  // :197-218
    s_nops = n;
    // :125-153: q[l] = 1, T[l] = 0, q[F - 1] = q[l] * Quaterniond(relative_R), T[F - 1] = relative_T; c_Quat = q.inverse(),
    // c_Rotation = c_Quat.toRotationMatrix(), c_Translation = -1 * (c_Rotation * T)
    const q4 ql = q4{1.0, 0.0, 0.0, 0.0};
    const q4 qn = qmul(ql, R2q(ldm(hd->relative_R)));
#pragma unroll
    for (int e = 0; e < 2; e++) {
      const int f = e == 0 ? l : F - 1;
      const q4 cq = qinv(e == 0 ? ql : qn);
      const d3 T = e == 0 ? mk3(0.0, 0.0, 0.0) : ld3(hd->relative_T);
      const m33 R = q2R(cq);
      const double t[3] = {-(R.a[0] * T.x + R.a[1] * T.y + R.a[2] * T.z), -(R.a[3] * T.x + R.a[4] * T.y + R.a[5] * T.z), -(R.a[6] * T.x + R.a[7] * T.y + R.a[8] * T.z)};
#pragma unroll
      for (int r = 0; r < 3; r++) {
        s_pose[f][4 * r] = R.a[3 * r], s_pose[f][4 * r + 1] = R.a[3 * r + 1], s_pose[f][4 * r + 2] = R.a[3 * r + 2], s_pose[f][4 * r + 3] = t[r];
        to[3 * f + r] = t[r];
      }
      qo[4 * f] = cq.w, qo[4 * f + 1] = cq.x, qo[4 * f + 2] = cq.y, qo[4 * f + 3] = cq.z;
      res->posed[f] = 1;
    }
  }
  for (int j = tid; j < P; j += NT) X[3 * j] = 0.0, X[3 * j + 1] = 0.0, X[3 * j + 2] = 0.0, tri_op[j] = -1;
  __syncthreads();

  const int nops = s_nops, per = (P + NT - 1) / NT;
  const int j0 = min(P, tid * per), j1 = min(P, j0 + per);  // this thread's block of points in a gather
  for (int op = 0; op < nops; op++) {
    const int kind = s_kind[op], a = s_a[op], b = s_b[op];
    if (kind == SFMCH_PNP) {
      // ---- solveFrameByPnP(a): gather in ascending j (solve_for_sign reads the first correspondence), then the pose
      int cnt = 0;
      for (int j = j0; j < j1; j++) cnt += (tri_op[j] >= 0 && slot[(size_t)j * F + a] >= 0) ? 1 : 0;
      s_scan[tid] = cnt;
      __syncthreads();
#pragma unroll
      for (int d = 1; d < NT; d <<= 1) {
        const int v = tid >= d ? s_scan[tid - d] : 0;
        __syncthreads();
        s_scan[tid] += v;
        __syncthreads();
      }
      int w = s_scan[tid] - cnt;
      const int n = s_scan[NT - 1];
      for (int j = j0; j < j1; j++) {
        const int o = slot[(size_t)j * F + a];
        if (tri_op[j] >= 0 && o >= 0) {
#pragma unroll
          for (int k = 0; k < 3; k++) gpw[3 * (size_t)w + k] = X[3 * (size_t)j + k], gus[3 * (size_t)w + k] = bearing[3 * (size_t)o + k];
          w++;
        }
      }
      if (tid == 0) {
        res->o.pnp_op[a] = op, res->o.pnp_count[a] = n;
        if (n < SFMCH_MIN_PNP) res->o.status = 1, res->o.failed_frame = a;  // :51-52
      }
      if (n < SFMCH_MIN_PNP) break;
      __syncthreads();
      PnpRecord *rec = (PnpRecord *)&res->o.pnp[a];
      pnp_pose(n, gpw, gus, gal, rec, red, ut, sbeta, tid);
      if (tid == 0) {  // :166-170 / :188-192; c_Quat[i] = c_Rotation[i] is Eigen's matrix to quaternion, reflection or not
        const int st = rec->status;
        s_flag = st;
        if (st != 0) {
          res->o.status = 2, res->o.failed_frame = a;
        } else {
#pragma unroll
          for (int r = 0; r < 3; r++) {
            s_pose[a][4 * r] = rec->R[3 * r], s_pose[a][4 * r + 1] = rec->R[3 * r + 1], s_pose[a][4 * r + 2] = rec->R[3 * r + 2], s_pose[a][4 * r + 3] = rec->T[r];
            to[3 * a + r] = rec->T[r];
          }
          const q4 cq = R2q(ldm(rec->R));
          qo[4 * a] = cq.w, qo[4 * a + 1] = cq.x, qo[4 * a + 2] = cq.y, qo[4 * a + 3] = cq.z;
          res->posed[a] = 1;
        }
      }
      __syncthreads();
      if (s_flag != 0) break;
    } else {
      // ---- triangulateTwoFrames(a, Pose[a], b, Pose[b]) or the closing loop (first and last observation of the point)
      for (int j = tid; j < P; j += NT) {
        if (tri_op[j] >= 0) continue;
        int o0, o1, f0 = a, f1 = b;
        if (kind == SFMCH_TRI) {
          o0 = slot[(size_t)j * F + a], o1 = slot[(size_t)j * F + b];
        } else {
          const int s = off[j], e = off[j + 1];
          o0 = e - s >= 2 ? s : -1, o1 = e - 1;
          f0 = frm[s], f1 = frm[e - 1];
        }
        if (o0 < 0 || o1 < 0) continue;
        const d3 p = sfmch_triangulate(s_pose[f0], s_pose[f1], ld3(bearing + 3 * (size_t)o0), ld3(bearing + 3 * (size_t)o1));
        X[3 * (size_t)j] = p.x, X[3 * (size_t)j + 1] = p.y, X[3 * (size_t)j + 2] = p.z;
        tri_op[j] = op;
      }
      __syncthreads();
    }
  }
}
