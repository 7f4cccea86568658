// kernels_trackbatch.h — the kernels of one frame (kernels_klt.h, kernels_clahe.h, kernels_track.h, kernels_gft.h,
// kernels_trackframe.h) with the slot in blockIdx.z, behind lfvio_track_batch_frame (include/lfvio.h, trackbatch.inc).  Every entry
// here does three things: it reads its slot's descriptor (TbSlot, trackbatch_plan.h) from the device array — uniform over the
// workgroup, so scalar loads — returns at once for an idle slot (and, in the rejection and the detection, for one that does not
// publish), and calls the SAME device function as the single kernel with what that function needs as plain arguments: the
// descriptor costs the bodies no LDS and no scratch, and a slot's bits are those of a context of its own by construction.
//
// Grids are sized by the batch's bounds (trackbatch_bounds): a workgroup beyond its own slot's count returns inside the body, as
// the k_*_n kernels' do for the single call.  Segments inside a slot's part of the staging block are laid out for the bounds too
// (TbStage); the scratch tables t1, t2 and the table that comes down are three arrays of n0_max / B_max entries.
//
//   k_tb_copy  : bytes from src + z * sstride to dst + z * dstride (the base mask into one slot or into all of them, the slots'
//                images into a larger block); k_tb_image: a slot's staged image into level 0 of its fresh pyramid.  Where the single
//                route asks the runtime for a device-to-device copy.  k_img_gray_b: the same place under lfvio_track_batch_format — the
//                staged image in its encoding into grey at level 0 (img_gray_body, kernels_imgfmt.h); the CLAHE kernels then read
//                level 0 (from_fresh) and the map equalizes it in place.
#pragma once
#include "kernels_clahe.h"
#include "kernels_imgfmt.h"
#include "kernels_remap.h"
#include "kernels_trackframe.h"
#include "kernels_tracksource.h"
#include "trackbatch_source_plan.h"

constexpr int TB_COPY_THREADS = 256, TB_COPY_BYTES = TB_COPY_THREADS * 16;

// This workgroup's slot: the descriptor's numbers (scalar loads: the index is uniform) and the slot's pointers, every one formed
// from a pointer ARGUMENT of the kernel — the compiler knows them to be global memory, as it knows the single kernels' arguments,
// and gives the bodies the same global instructions on a scalar base.  (A pointer read from the descriptor would be a generic one:
// flat instructions with the address in vector registers; k_tf_finish's body took 50 VGPRs that way against 26.)
struct TbView {
  int active, publish, n0, n_id, prev_count, prev_built;
  double dt;
  const TrackCam *cam;
  const unsigned char *image, *base;
  const unsigned *words;
  unsigned char *fresh, *prev;
  char *work, *clahe, *have, *next, *next_map, *mid, *down;
  const char *prev_map;
};
DEV TbView tb_view(const TbSlot *slots, const TbMem &m, const TbStage &o) {
  const size_t z = blockIdx.z;
  const TbSlot &d = slots[z];
  TbView s;
  s.active = d.active, s.publish = d.publish, s.n0 = d.n0, s.n_id = d.n_id, s.prev_count = d.prev_count, s.prev_built = d.prev_built, s.dt = d.dt;
  s.cam = &d.cam;
  char *img = m.image + z * m.image_stride, *fix = m.fixed + z * TB_FIXED_BYTES;
  s.image = (const unsigned char *)(m.stage + m.images_at + (size_t)d.image_k * m.images_stride);
  s.words = (const unsigned *)(m.stage + m.words_at + (size_t)d.words_k * m.words_stride);
  s.fresh = (unsigned char *)(img + (size_t)(1 - d.pcur) * m.pyr);
  s.prev = d.same ? (unsigned char *)(img + (size_t)d.pcur * m.pyr) : s.fresh;
  s.base = d.masked ? (const unsigned char *)(img + m.mask_at) : nullptr;
  s.work = img + m.work_at;
  s.clahe = m.clahe + z * m.clahe_stride;
  s.have = fix + trackbatch_table_at(d.tcur), s.next = fix + trackbatch_table_at(1 - d.tcur);
  s.prev_map = fix + trackbatch_map_at(d.mcur), s.next_map = fix + trackbatch_map_at(1 - d.mcur);
  s.mid = m.stage + o.mid + z * o.mid_stride, s.down = m.stage + o.down + z * o.down_stride;
  return s;
}

// src and dst 16-aligned
DEV void tb_copy_body(const unsigned char *src, unsigned char *dst, size_t bytes) {
  const size_t at = ((size_t)blockIdx.x * TB_COPY_THREADS + threadIdx.x) * 16;
  if (at + 16 <= bytes)
    *(uint4 *)(dst + at) = *(const uint4 *)(src + at);
  else
    for (size_t i = at; i < bytes; i++) dst[i] = src[i];
}
__global__ __launch_bounds__(TB_COPY_THREADS) void k_tb_copy(const unsigned char *src, size_t sstride, unsigned char *dst, size_t dstride, size_t bytes) {
  tb_copy_body(src + blockIdx.z * sstride, dst + blockIdx.z * dstride, bytes);
}
__global__ __launch_bounds__(TB_COPY_THREADS) void k_tb_image(const TbSlot *slots, TbMem m, TbStage o, size_t bytes) {
  const TbView s = tb_view(slots, m, o);
  if (!s.active) return;
  tb_copy_body(s.image, s.fresh, bytes);
}

__global__ __launch_bounds__(IMG_THREADS) void k_img_gray_b(const TbSlot *slots, TbMem m, TbStage o, int code, size_t step, int W, int H) {
  const TbView s = tb_view(slots, m, o);
  if (!s.active) return;
  img_gray_body(code, s.image, step, s.fresh, W, H);
}

// ---- the slots' resident remaps (lfvio_track_batch_map / lfvio_track_batch_source).  A slot's maps lie at m.maps +
// slot * m.maps_stride: [map_x | map_y at maps_y_at | the integer map at maps_index_at] (TbMaps, trackbatch_plan.h, which states the
// alignment the int4 load and the dword store rest on).
//   k_remap_gray_b : where k_img_gray_b / k_tb_image stand while the setting is on — the staged SOURCE image gathered through the
//                    slot's own integer map into grey at level 0 of its fresh pyramid (remap_gray_body, kernels_tracksource.h).
//                    Grid remap_apply_blocks(W * H) x 1 x slots.  Bounds: every entry of an active slot's integer map was written for
//                    the staged images' geometry (the host rebuilds them first where it was not), so offset + BPP <= src_height *
//                    step, the bytes of one staged image; W * H pixels is the size of every active slot's map (the call's check).
//   k_remap_build_b: k_remap_build for slots first .. first + gridDim.z - 1, the same recipe in each: one launch for slot = -1.
//                    There are no descriptors on the device outside a frame: the slot is first + blockIdx.z.
//   k_remap_index_b: the integer maps of ALL mapped slots (map_px != 0 in the descriptor, idle ones too) from their float maps for
//                    another source geometry, in one launch; grid.x covers the largest map, a lane past its own slot's returns.
template <int BPP>
__global__ __launch_bounds__(REMAP_THREADS) void k_remap_gray_b(const TbSlot *slots, TbMem m, TbStage o, int code, size_t pixels) {
  const TbView s = tb_view(slots, m, o);
  if (!s.active) return;
  remap_gray_body<BPP>(code, (const int *)(m.maps + (size_t)blockIdx.z * m.maps_stride + m.maps_index_at), s.image, s.fresh, pixels);
}
__global__ __launch_bounds__(REMAP_THREADS) void k_remap_build_b(RemapBuildArgs a, TbMem m, int first) {
  char *maps = m.maps + ((size_t)first + blockIdx.z) * m.maps_stride;
  remap_build_body(a, (float *)maps, (float *)(maps + m.maps_y_at), (int *)(maps + m.maps_index_at));
}
__global__ __launch_bounds__(REMAP_THREADS) void k_remap_index_b(const TbSlot *slots, TbMem m, RemapGeom g) {
  const int px = slots[blockIdx.z].map_px;
  if (!px) return;
  char *maps = m.maps + (size_t)blockIdx.z * m.maps_stride;
  remap_index_body(g, (size_t)px, (const float *)maps, (const float *)(maps + m.maps_y_at), (int *)(maps + m.maps_index_at));
}
// code: one of image_format.h's table (the host has checked it)
inline void remap_gray_b_launch(hipStream_t fs, unsigned slots_z, const TbSlot *slots, const TbMem &m, const TbStage &o, int code, size_t pixels) {
  const dim3 grid(remap_apply_blocks(pixels), 1, slots_z), block(REMAP_THREADS);
  switch (imgfmt_bpp(code)) {
    case 1: hipLaunchKernelGGL(k_remap_gray_b<1>, grid, block, 0, fs, slots, m, o, code, pixels); break;
    case 2: hipLaunchKernelGGL(k_remap_gray_b<2>, grid, block, 0, fs, slots, m, o, code, pixels); break;
    case 3: hipLaunchKernelGGL(k_remap_gray_b<3>, grid, block, 0, fs, slots, m, o, code, pixels); break;
    default: hipLaunchKernelGGL(k_remap_gray_b<4>, grid, block, 0, fs, slots, m, o, code, pixels); break;
  }
}

// ---- CLAHE: the staged image (from_fresh: the grey image k_img_gray_b or k_remap_gray_b left at level 0) into level 0 of the fresh pyramid
__global__ __launch_bounds__(CLAHE_THREADS) void k_clahe_hist_b(const TbSlot *slots, TbMem m, TbStage o, int from_fresh, int W, int H, int tiles_x, int tw, int th) {
  const TbView s = tb_view(slots, m, o);
  if (!s.active) return;
  clahe_hist_body(from_fresh ? (const unsigned char *)s.fresh : s.image, W, H, tiles_x, tw, th, (int *)s.clahe);
}
__global__ __launch_bounds__(CLAHE_THREADS) void k_clahe_lut_b(const TbSlot *slots, TbMem m, TbStage o, int clip, float lut_scale, size_t lut_at) {
  const TbView s = tb_view(slots, m, o);
  if (!s.active) return;
  clahe_lut_body((int *)s.clahe, clip, lut_scale, (unsigned char *)s.clahe + lut_at);
}
template <bool VEC>
__global__ __launch_bounds__(CLAHE_THREADS) void k_clahe_map_b(const TbSlot *slots, TbMem m, TbStage o, int from_fresh, int W, int H, int tiles_x, int tiles_y, int th, int sub,
                                                               float inv_tw, float inv_th, size_t lut_at) {
  const TbView s = tb_view(slots, m, o);
  if (!s.active) return;
  clahe_map_body<VEC>(from_fresh ? (const unsigned char *)s.fresh : s.image, s.fresh, W, H, tiles_x, tiles_y, th, sub, inv_tw, inv_th, (const unsigned char *)s.clahe + lut_at);
}

// ---- the flow.  resident == 0: level k of the fresh pyramid; 1: of the resident one, where an earlier call built fewer levels
__global__ __launch_bounds__(256) void k_klt_down_b(const TbSlot *slots, TbMem m, TbStage o, int resident, int k, size_t src_at, int sw, int sh, size_t dst_at, int dw, int dh) {
  const TbView s = tb_view(slots, m, o);
  if (!s.active) return;
  if (resident && (s.prev == s.fresh || k <= s.prev_built)) return;
  unsigned char *pyr = resident ? s.prev : s.fresh;
  klt_down_body(pyr + src_at, sw, sh, pyr + dst_at, dw, dh);
}
__global__ __launch_bounds__(KLT_THREADS) void k_klt_track_b(const TbSlot *slots, TbMem m, TbStage o, KltArgs a) {
  const TbView s = tb_view(slots, m, o);
  if (!s.active) return;
  klt_track_body(a, s.n0, s.prev, s.fresh, (const float *)s.have, (float *)(s.mid + o.next), (unsigned char *)(s.mid + o.status), nullptr);
}

// ---- reduceVector and the rejection
__global__ __launch_bounds__(TF_THREADS) void k_tf_flow_b(const TbSlot *slots, TbMem m, TbStage o, int n0_max, int S) {
  const TbView s = tb_view(slots, m, o);
  if (!s.active) return;
  const TfTable have = tf_table(s.have, LFVIO_TRACK_MAX_POINTS);
  tf_flow_body(s.n0, (const unsigned char *)(s.mid + o.status), have.pts, (const float *)(s.mid + o.next), have.ids, have.cnt, (float *)(s.mid + o.c1),
               tf_table(s.mid + o.t1, n0_max), (TfDev *)(s.down + o.dev), S, s.publish ? s.words : nullptr, (int *)(s.mid + o.samples));
}
__global__ __launch_bounds__(TRK_THREADS) void k_trk_lift_b(const TbSlot *slots, TbMem m, TbStage o) {
  const TbView s = tb_view(slots, m, o);
  if (!s.active || !s.publish || s.n0 < TRACK_MIN_MATCHES) return;
  trk_lift_body(*s.cam, ((const TfDev *)(s.down + o.dev))->n1, (const float *)(s.mid + o.c1), (const float *)(s.mid + o.t1), (double *)(s.mid + o.bl),
                (double *)(s.mid + o.br));
}
__global__ __launch_bounds__(TV_HYP_THREADS) void k_tv_hyp_b(const TbSlot *slots, TbMem m, TbStage o) {
  __shared__ double s2[TV_CHUNK], s1[TV_CHUNK];
  const TbView s = tb_view(slots, m, o);
  if (!s.active || !s.publish || s.n0 < TRACK_MIN_MATCHES) return;
  const int N = ((const TfDev *)(s.down + o.dev))->n1, k = blockIdx.x;
  if (N < TRACK_MIN_MATCHES) return;
  tv_hyp_body(N, (const double *)(s.mid + o.bl), (const double *)(s.mid + o.br), (const int *)(s.mid + o.samples) + 8 * (size_t)k,
              (double *)(s.mid + o.E) + 9 * (size_t)k, (float *)(s.mid + o.score) + k, s2, s1, threadIdx.x);
}
__global__ __launch_bounds__(TV_FIT_THREADS) void k_trk_fit_b(const TbSlot *slots, TbMem m, TbStage o, int S) {
  __shared__ TvFitLds lds;
  const TbView s = tb_view(slots, m, o);
  if (!s.active || !s.publish) return;
  TfDev *dev = (TfDev *)(s.down + o.dev);
  trk_fit_n_body(dev->n1, S, (const double *)(s.mid + o.bl), (const double *)(s.mid + o.br), (const double *)(s.mid + o.E), (const float *)(s.mid + o.score),
                 (double *)(s.mid + o.A), (unsigned char *)(s.mid + o.mask), &dev->reject, lds);
}
__global__ __launch_bounds__(TF_THREADS) void k_tf_reject_b(const TbSlot *slots, TbMem m, TbStage o, int n0_max) {
  const TbView s = tb_view(slots, m, o);
  if (!s.active || !s.publish) return;
  tf_reject_body((const unsigned char *)(s.mid + o.mask), tf_table(s.mid + o.t1, n0_max), tf_table(s.mid + o.t2, n0_max), (TfDev *)(s.down + o.dev));
}

// ---- setMask and goodFeaturesToTrack on level 0 of the fresh pyramid
__global__ __launch_bounds__(GFT_THREADS) void k_gft_thin_b(const TbSlot *slots, TbMem m, TbStage o, GftOffsets wk, int n0_max, int W, int H, int r) {
  const TbView s = tb_view(slots, m, o);
  if (!s.active || !s.publish) return;
  const TfTable t2 = tf_table(s.mid + o.t2, n0_max);
  gft_thin_body(((const TfDev *)(s.down + o.dev))->n2, t2.pts, t2.cnt, s.base, W, H, r, (GftDev *)(s.work + wk.st), (int *)(s.mid + o.kept),
                (int *)(s.work + wk.kxy));
}
__global__ __launch_bounds__(GFT_THREADS) void k_gft_response_b(const TbSlot *slots, TbMem m, TbStage o, GftOffsets wk, int W, int H, int r, int max_count) {
  const TbView s = tb_view(slots, m, o);
  if (!s.active || !s.publish) return;
  gft_response_body(s.fresh, W, H, s.base, (const int *)(s.work + wk.kxy), r, max_count, (GftDev *)(s.work + wk.st), (double *)(s.work + wk.lam),
                    (unsigned char *)(s.work + wk.mask));
}
__global__ __launch_bounds__(GFT_THREADS) void k_gft_cand_b(const TbSlot *slots, TbMem m, TbStage o, GftOffsets wk, int W, int H, double quality, int max_count) {
  const TbView s = tb_view(slots, m, o);
  if (!s.active || !s.publish) return;
  gft_cand_body((const double *)(s.work + wk.lam), (const unsigned char *)(s.work + wk.mask), W, H, quality, max_count, (GftDev *)(s.work + wk.st),
                (unsigned long long *)(s.work + wk.keys), (unsigned *)(s.work + wk.idx));
}
__global__ __launch_bounds__(GFT_SORT_THREADS) void k_gft_sort_local_b(const TbSlot *slots, TbMem m, TbStage o, GftOffsets wk, unsigned stage) {
  const TbView s = tb_view(slots, m, o);
  if (!s.active || !s.publish) return;
  gft_sort_local_body((const GftDev *)(s.work + wk.st), (unsigned long long *)(s.work + wk.keys), (unsigned *)(s.work + wk.idx), stage);
}
__global__ __launch_bounds__(GFT_THREADS) void k_gft_sort_global_b(const TbSlot *slots, TbMem m, TbStage o, GftOffsets wk, unsigned k, unsigned j) {
  const TbView s = tb_view(slots, m, o);
  if (!s.active || !s.publish) return;
  gft_sort_global_body((const GftDev *)(s.work + wk.st), (unsigned long long *)(s.work + wk.keys), (unsigned *)(s.work + wk.idx), k, j);
}
__global__ __launch_bounds__(GFT_THREADS) void k_gft_pick_b(const TbSlot *slots, TbMem m, TbStage o, GftOffsets wk, int W, int d, int max_count) {
  const TbView s = tb_view(slots, m, o);
  if (!s.active || !s.publish) return;
  gft_pick_body((const GftDev *)(s.work + wk.st), (const unsigned *)(s.work + wk.idx), W, d, max_count, (float *)(s.mid + o.corners),
                &((TfDev *)(s.down + o.dev))->detect);
}

// ---- the next table, undistortedPoints, the message
__global__ __launch_bounds__(TF_THREADS) void k_tf_finish_b(const TbSlot *slots, TbMem m, TbStage o, int n0_max, int B_max) {
  const TbView s = tb_view(slots, m, o);
  if (!s.active) return;
  tf_finish_body(s.publish, tf_table(s.mid + (s.publish ? o.t2 : o.t1), n0_max), (const int *)(s.mid + o.kept), (const float *)(s.mid + o.corners), s.n_id,
                 tf_table(s.next, LFVIO_TRACK_MAX_POINTS), tf_table(s.down + o.table, B_max), (int *)(s.mid + o.raw), (TfDev *)(s.down + o.dev));
}
__global__ __launch_bounds__(TRK_THREADS) void k_trk_undist_b(const TbSlot *slots, TbMem m, TbStage o) {
  __shared__ int sid[LFVIO_TRACK_MAX_POINTS];
  const TbView s = tb_view(slots, m, o);
  if (!s.active) return;
  const int N = ((const TfDev *)(s.down + o.dev))->num_points;
  if ((int)(blockIdx.x * TRK_THREADS) >= N) return;
  trk_undist_body(*s.cam, N, (const float *)(s.down + o.table), (const int *)(s.mid + o.raw), s.dt, s.prev_count, (const int *)s.prev_map,
                  (const float *)(s.prev_map + TRACK_MAP_IDS), (float *)(s.down + o.un), (float *)(s.down + o.un3d), (float *)(s.down + o.vel),
                  (int *)(s.mid + o.matched), (int *)s.next_map, (float *)(s.next_map + TRACK_MAP_IDS), sid);
}
__global__ __launch_bounds__(TF_THREADS) void k_tf_message_b(const TbSlot *slots, TbMem m, TbStage o, int B_max) {
  const TbView s = tb_view(slots, m, o);
  if (!s.active || !s.publish) return;
  tf_message_body((const TfDev *)(s.down + o.dev), B_max, tf_table(s.down + o.table, B_max), (const float *)(s.down + o.un3d), (const float *)(s.down + o.vel),
                  (int *)(s.down + o.msg), (float *)(s.down + o.msg + TF_MSG_HEAD));
}
