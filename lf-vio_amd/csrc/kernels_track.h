// kernels_track.h — the two steps of FeatureTracker::readImage that need the camera (feature_tracker/src/feature_tracker.cpp):
// rejectWithF (:329-386) behind lfvio_track_reject and undistortedPoints (:441-504) behind lfvio_track_undistort, with
// the lift of four camera models as device functions: OCAMCamera::liftProjective (ScaramuzzaCamera.cc:623-645),
// PinholeCamera::liftProjective (PinholeCamera.cc:450-510), CataCamera::liftProjective (CataCamera.cc:556-626) and
// EquidistantCamera::liftProjective (EquidistantCamera.cc:428-442, restated in camera_kb.h).  The specification is in include/lfvio.h
// and, as numpy, in tests/track_ref.py (OCam), tests/camera_ref.py (PINHOLE, MEI) and tests/kb_ref.py (KANNALA_BRANDT).
//
//   k_trk_lift   : a thread per point of BOTH sets (2 N threads): the unit bearing of cur_pts[i] / forw_pts[i] in double, into the
//                  staging block where k_tv_hyp (kernels_twoview.h, reused as it is) and k_trk_fit read them.
//   k_trk_fit    : one workgroup of TV_FIT_THREADS: tv_fit_body<false, true> — selection, refit, mask, and nothing behind the mask.
//                  Writes LfvioTrackRejectOut and, on the no-model paths, status[] = 1 throughout: the host copies one block down
//                  whatever happened.
//   k_trk_undist : a thread per point: the lift, un_pts, un_pts_3d, the lookup of the id among the PREVIOUS call's ids and the
//                  velocity.  The previous ids are staged in LDS (4096 ints) and every thread walks ALL of them for the smallest
//                  matching index — the same trip count in every lane, an LDS broadcast per step, and ids == -1 only discards the
//                  result behind the loop, so nothing diverges.  At N <= 4096 this is cheaper than sorting.  The new (id, un_pts_3d)
//                  pairs go to the OTHER resident map; the previous one is only read.
//
//   k_*_n        : the same bodies with N read from the device (and k_tv_hyp_n around tv_hyp_body) for lfvio_track_frame
//                  (trackframe.inc), whose host knows only a bound of N and sizes the grid for it.  They take the cases the host
//                  filters for the kernels above: N < 8 in the rejection (status 2, no sample index is read), N = 0 in
//                  k_trk_undist_n (a workgroup without a point returns before any load).
//
// The lift is written operation by operation and the library is built with -ffp-contract=off: every product and sum is rounded on
// its own, as the restatement's are.  The norm is sqrt((x x + y y) + z z), left to right as tv_residual forms its norms; Eigen's
// own reduction may order the terms differently (the reference does not build here, so the two were never compared).
#pragma once
#include "kernels_twoview.h"
#include "track_plan.h"

constexpr int TRK_THREADS = 256;

// PinholeCamera::distortion (PinholeCamera.cc:646-662; CataCamera's is the same text): grouped as include/lfvio.h states it
DEV void trk_distortion(const TrackCam &cam, double x, double y, double &dx, double &dy) {
  const double mx2 = x * x, my2 = y * y, mxy = x * y, rho2 = mx2 + my2;
  const double rad = cam.k1 * rho2 + (cam.k2 * rho2) * rho2;
  dx = (x * rad + (2.0 * cam.p1) * mxy) + cam.p2 * (rho2 + 2.0 * mx2);
  dy = (y * rad + (2.0 * cam.p2) * mxy) + cam.p1 * (rho2 + 2.0 * my2);
}

// The part both liftProjective share (PinholeCamera.cc:456-506, CataCamera.cc:562-612): the normalised plane and the recursive
// distortion model, n = 8 evaluations.  The trip count is fixed, so nothing diverges within a wave.
DEV void trk_undistorted_plane(const TrackCam &cam, float px, float py, double &mx_u, double &my_u) {
  const double mx_d = cam.inv11 * (double)px + cam.inv13, my_d = cam.inv22 * (double)py + cam.inv23;
  mx_u = mx_d, my_u = my_d;
  if (cam.no_distortion) return;
  for (int i = 0; i < 8; i++) {
    double dx, dy;
    trk_distortion(cam, mx_u, my_u, dx, dy);
    mx_u = mx_d - dx, my_u = my_d - dy;
  }
}

// PinholeCamera::liftProjective (:450-510)
DEV d3 trk_lift_pinhole(const TrackCam &cam, float px, float py) {
  double mx_u, my_u;
  trk_undistorted_plane(cam, px, py, mx_u, my_u);
  return mk3(mx_u, my_u, 1.0);
}

// CataCamera::liftProjective (:556-626)
DEV d3 trk_lift_mei(const TrackCam &cam, float px, float py) {
  double mx_u, my_u;
  trk_undistorted_plane(cam, px, py, mx_u, my_u);
  if (cam.xi == 1.0) return mk3(mx_u, my_u, ((1.0 - mx_u * mx_u) - my_u * my_u) / 2.0);  // :618
  const double rho2 = mx_u * mx_u + my_u * my_u;
  return mk3(mx_u, my_u, 1.0 - (cam.xi * (rho2 + 1.0)) / (cam.xi + sqrt(1.0 + (1.0 - cam.xi * cam.xi) * rho2)));  // :624
}

// EquidistantCamera::liftProjective as camera_kb.h restates it: the normalised plane, the root by a fixed count of Newton steps, sin
// and cos by the header's own routine, the bearing.  No trip count depends on the data.
DEV d3 trk_lift_kb(const TrackCam &cam, float px, float py) {
  d3 P;
  kb_lift_pixel(cam.inv11, cam.inv13, cam.inv22, cam.inv23, cam.poly, cam.theta_lim, cam.r_lim, px, py, P.x, P.y, P.z);
  return P;
}

// liftProjective of the pixel (px, py).  The model is the same in every thread of a workgroup (a kernel argument, or the slot's
// camera in the batched route), so the branches below are uniform.  OCAMCamera::liftProjective:
DEV d3 trk_lift(const TrackCam &cam, float px, float py) {
  if (cam.model == LFVIO_CAM_PINHOLE) return trk_lift_pinhole(cam, px, py);
  if (cam.model == LFVIO_CAM_MEI) return trk_lift_mei(cam, px, py);
  if (cam.model == LFVIO_CAM_KANNALA_BRANDT) return trk_lift_kb(cam, px, py);
  const double x = (double)px - cam.cx, y = (double)py - cam.cy;  // :627
  const double xa = cam.inv_scale * (x - cam.d * y), ya = cam.inv_scale * (-cam.e * x + cam.c * y);  // :631-632
  const double phi = sqrt(xa * xa + ya * ya);
  double p = 1.0, z = 0.0;
#pragma unroll
  for (int i = 0; i < 5; i++) {  // :638-642
    z += p * cam.poly[i];
    p *= phi;
  }
  return mk3(xa, ya, -z);  // :644
}

DEV double trk_norm(d3 P) { return sqrt((P.x * P.x + P.y * P.y) + P.z * P.z); }

DEV void trk_lift_body(const TrackCam &cam, int N, const float *cur, const float *forw, double *bl, double *br) {
  const int t = blockIdx.x * TRK_THREADS + threadIdx.x;
  if (t >= 2 * N) return;
  const bool second = t >= N;
  const int i = second ? t - N : t;
  const float *px = (second ? forw : cur) + 2 * (size_t)i;
  const d3 P = trk_lift(cam, px[0], px[1]);
  const double n = trk_norm(P);
  double *b = (second ? br : bl) + 3 * (size_t)i;
  b[0] = P.x / n, b[1] = P.y / n, b[2] = P.z / n;  // :343, :353
}
__global__ __launch_bounds__(TRK_THREADS) void k_trk_lift(TrackCam cam, int N, const float *cur, const float *forw, double *bl, double *br) {
  trk_lift_body(cam, N, cur, forw, bl, br);
}
// N from the device (lfvio_track_frame): the grid is the host's bound of it
__global__ __launch_bounds__(TRK_THREADS) void k_trk_lift_n(TrackCam cam, const int *N, const float *cur, const float *forw, double *bl, double *br) {
  trk_lift_body(cam, *N, cur, forw, bl, br);
}

// One workgroup.  out is written on every path (E only with status 0); status[0 .. N) too.
DEV void trk_fit_body(int N, int S, const double *bl, const double *br, const double *E_all, const float *score_all, double *A,
                      unsigned char *status, LfvioTrackRejectOut *out, TvFitLds &lds) {
  TvFit f;
  const int st = tv_fit_body<false, true>(N, S, bl, br, E_all, score_all, A, status, lds, f);  // (the same in every thread)
  if (st != 0)
    for (int i = threadIdx.x; i < N; i += TV_FIT_THREADS) status[i] = 1;
  if (threadIdx.x != 0) return;
  out->status = st, out->best_sample = f.best, out->num_inliers = f.n_in, out->best_score = f.best_score;
  if (st == 0) {
#pragma unroll
    for (int j = 0; j < 9; j++) out->E[j] = f.E[j];
  }
}
__global__ __launch_bounds__(TV_FIT_THREADS) void k_trk_fit(int N, int S, const double *bl, const double *br, const double *E_all,
                                                            const float *score_all, double *A, unsigned char *status, LfvioTrackRejectOut *out) {
  __shared__ TvFitLds lds;
  trk_fit_body(N, S, bl, br, E_all, score_all, A, status, out, lds);
}
// N from the device.  N < 8 is lfvio_track_reject's host branch (:331), which the host cannot take here: status 2, nothing rejected,
// and no bearing, hypothesis or sample index is read (k_tv_hyp_n has not run).
DEV void trk_fit_n_body(int N, int S, const double *bl, const double *br, const double *E_all, const float *score_all, double *A,
                        unsigned char *status, LfvioTrackRejectOut *out, TvFitLds &lds) {
  if (N < TRACK_MIN_MATCHES) {
    for (int i = threadIdx.x; i < N; i += TV_FIT_THREADS) status[i] = 1;
    if (threadIdx.x == 0) out->status = 2, out->best_sample = -1, out->num_inliers = 0, out->best_score = 0.0;
    return;
  }
  trk_fit_body(N, S, bl, br, E_all, score_all, A, status, out, lds);
}
__global__ __launch_bounds__(TV_FIT_THREADS) void k_trk_fit_n(const int *Np, int S, const double *bl, const double *br, const double *E_all,
                                                              const float *score_all, double *A, unsigned char *status, LfvioTrackRejectOut *out) {
  __shared__ TvFitLds lds;
  trk_fit_n_body(*Np, S, bl, br, E_all, score_all, A, status, out, lds);
}
// k_tv_hyp (kernels_twoview.h) with N from the device; N < 8: no sample set was drawn
__global__ __launch_bounds__(TV_HYP_THREADS) void k_tv_hyp_n(const int *Np, const double *bl, const double *br, const int *samples, double *E_all,
                                                             float *score_all) {
  __shared__ double s2[TV_CHUNK], s1[TV_CHUNK];
  const int N = *Np, k = blockIdx.x;
  if (N < TRACK_MIN_MATCHES) return;
  tv_hyp_body(N, bl, br, samples + 8 * (size_t)k, E_all + 9 * (size_t)k, score_all + k, s2, s1, threadIdx.x);
}

// grid ceil(N / 256).  prev_ids / prev_3d: the P pairs of the previous call (P = 0: the map is empty, every velocity is 0);
// new_ids / new_3d: this call's, for the next one.
DEV void trk_undist_body(const TrackCam &cam, int N, const float *pts, const int *ids, double dt, int P, const int *prev_ids,
                         const float *prev_3d, float *un, float *un3d, float *vel, int *matched, int *new_ids, float *new_3d, int *sid) {
  const int tid = threadIdx.x, i = blockIdx.x * TRK_THREADS + tid;
  for (int j = tid; j < P; j += TRK_THREADS) sid[j] = prev_ids[j];
  __syncthreads();
  const bool live = i < N;
  const int ii = live ? i : N - 1;  // (N >= 1: the grid is empty otherwise) idle threads of the last block walk along, store nothing
  const int id = ids[ii];
  const d3 Q = trk_lift(cam, pts[2 * (size_t)ii], pts[2 * (size_t)ii + 1]);
  const double n = trk_norm(Q);
  const float ux = (float)(Q.x / Q.z), uy = (float)(Q.y / Q.z);                        // :454
  const float bx = (float)(Q.x / n), by = (float)(Q.y / n), bz = (float)(Q.z / n);      // :455
  int best = P;  // the first occurrence wins (std::map::insert, :457-458)
  for (int j = P - 1; j >= 0; j--) best = sid[j] == id ? j : best;
  const bool found = id != -1 && best < P;  // -1 is never looked up (:471)
  float vx = 0.0f, vy = 0.0f, vz = 0.0f;
  if (found) {
    const float *q = prev_3d + 3 * (size_t)best;
    vx = (float)((double)(bx - q[0]) / dt);  // :478-481: the difference in float, the quotient in double
    vy = (float)((double)(by - q[1]) / dt);
    vz = (float)((double)(bz - q[2]) / dt);
  }
  if (!live) return;
  un[2 * (size_t)i] = ux, un[2 * (size_t)i + 1] = uy;
  un3d[3 * (size_t)i] = bx, un3d[3 * (size_t)i + 1] = by, un3d[3 * (size_t)i + 2] = bz;
  vel[3 * (size_t)i] = vx, vel[3 * (size_t)i + 1] = vy, vel[3 * (size_t)i + 2] = vz;
  matched[i] = found ? best : -1;
  new_ids[i] = id;
  new_3d[3 * (size_t)i] = bx, new_3d[3 * (size_t)i + 1] = by, new_3d[3 * (size_t)i + 2] = bz;
}
__global__ __launch_bounds__(TRK_THREADS) void k_trk_undist(TrackCam cam, int N, const float *pts, const int *ids, double dt, int P,
                                                            const int *prev_ids, const float *prev_3d, float *un, float *un3d, float *vel,
                                                            int *matched, int *new_ids, float *new_3d) {
  __shared__ int sid[LFVIO_TRACK_MAX_POINTS];
  trk_undist_body(cam, N, pts, ids, dt, P, prev_ids, prev_3d, un, un3d, vel, matched, new_ids, new_3d, sid);
}
// N from the device, the grid sized for the host's bound of it.  A workgroup with no point of its own returns before any load: with
// N = 0 the clamp `ii = N - 1` of the body would read index -1.
__global__ __launch_bounds__(TRK_THREADS) void k_trk_undist_n(TrackCam cam, const int *Np, const float *pts, const int *ids, double dt, int P,
                                                              const int *prev_ids, const float *prev_3d, float *un, float *un3d, float *vel,
                                                              int *matched, int *new_ids, float *new_3d) {
  __shared__ int sid[LFVIO_TRACK_MAX_POINTS];
  const int N = *Np;
  if ((int)(blockIdx.x * TRK_THREADS) >= N) return;
  trk_undist_body(cam, N, pts, ids, dt, P, prev_ids, prev_3d, un, un3d, vel, matched, new_ids, new_3d, sid);
}
