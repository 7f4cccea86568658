// kernels_track.h — the kernels of the two steps of FeatureTracker::readImage that need the camera (feature_tracker/src/feature_tracker.cpp):
// rejectWithF (:329-386) behind lfvio_track_reject and undistortedPoints (:441-504) behind lfvio_track_undistort.  Kernels only: the
// lift of the four camera models, the norm, the bearing and the float outputs of undistortedPoints are camera_models.h's host-and-device
// functions (cam_bearing, cam_undistorted), tested there on the CPU; the specification is in include/lfvio.h.
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
#pragma once
#include "kernels_twoview.h"
#include "track_plan.h"

constexpr int TRK_THREADS = 256;

DEV void trk_lift_body(const TrackCam &cam, int N, const float *cur, const float *forw, double *bl, double *br) {
  const int t = blockIdx.x * TRK_THREADS + threadIdx.x;
  if (t >= 2 * N) return;
  const bool second = t >= N;
  const int i = second ? t - N : t;
  const float *px = (second ? forw : cur) + 2 * (size_t)i;
  cam_bearing(cam, px[0], px[1], (second ? br : bl) + 3 * (size_t)i);
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
  const CamUndistorted u = cam_undistorted(cam, pts[2 * (size_t)ii], pts[2 * (size_t)ii + 1]);  // un_pts, un_pts_3d
  int best = P;  // the first occurrence wins (std::map::insert, :457-458)
  for (int j = P - 1; j >= 0; j--) best = sid[j] == id ? j : best;
  const bool found = id != -1 && best < P;  // -1 is never looked up (:471)
  float vx = 0.0f, vy = 0.0f, vz = 0.0f;
  if (found) {
    const float *q = prev_3d + 3 * (size_t)best;
    vx = (float)((double)(u.bx - q[0]) / dt);  // :478-481: the difference in float, the quotient in double
    vy = (float)((double)(u.by - q[1]) / dt);
    vz = (float)((double)(u.bz - q[2]) / dt);
  }
  if (!live) return;
  un[2 * (size_t)i] = u.ux, un[2 * (size_t)i + 1] = u.uy;
  un3d[3 * (size_t)i] = u.bx, un3d[3 * (size_t)i + 1] = u.by, un3d[3 * (size_t)i + 2] = u.bz;
  vel[3 * (size_t)i] = vx, vel[3 * (size_t)i + 1] = vy, vel[3 * (size_t)i + 2] = vz;
  matched[i] = found ? best : -1;
  new_ids[i] = id;
  new_3d[3 * (size_t)i] = u.bx, new_3d[3 * (size_t)i + 1] = u.by, new_3d[3 * (size_t)i + 2] = u.bz;
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
