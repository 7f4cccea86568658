// kernels_remap.h — the kernels behind lfvio_cam_project / lfvio_remap_build / lfvio_remap_apply (include/lfvio.h).  The
// arithmetic of a point and of a map entry is cam_project (camera_models.h) and remap_entry / remap_offset (remap_plan.h), the text the
// host compiles too; the camera's model and the map's kind are kernel arguments, so every branch on them is uniform.
//
//   k_cam_project    a lane per point: 3 doubles in, 2 out.
//   k_remap_build    a lane per output pixel, 32 x 8 tiles: the ray, its pixel, the two float map entries and — where the context
//                    knows the source images' geometry (g.bpp != 0) — the INTEGER map's entry: the source pixel's byte offset, or -1
//                    outside.  Once per map.
//   k_remap_index    the integer map alone from the float maps, for a source of another width, height, step or pixel size.
//   k_remap_apply    the per-image path: a gather bound by memory traffic — per output pixel 4 bytes of integer map (no rounding, and
//                    half the float maps' 8), BPP bytes gathered, BPP written.  Output and map are contiguous, so the image is one run
//                    of width * height pixels; a lane takes 4 consecutive ones: one 16-byte load of the map, 4 * BPP byte loads, and
//                    BPP whole dwords stored at a 4-aligned offset (mono8 one dword, bgr8 three, 16-bit two, four-byte pixels four)
//                    whatever the row's byte length is; the run's last fewer-than-4 pixels go byte by byte.  Neighbouring output
//                    pixels gather from neighbouring source pixels on smooth maps, so the caches see the reuse; the source is not
//                    staged in LDS (nothing measured asks for it).  An outside pixel still loads — byte 0 .. BPP - 1 of the source,
//                    which every source has — and selects zero, so no load hangs on a branch.
//   Bounds: an offset is sy * step + sx * BPP with sx < sw, sy < sh, step >= sw * BPP, so offset + BPP <= sh * step, the bytes uploaded;
//   lanes past the last pixel return before any access; `out` and the integer map come from allocations aligned to 256 bytes.
#pragma once
#include "dev_math.h"
#include "remap_plan.h"

__global__ __launch_bounds__(REMAP_PROJECT_THREADS) void k_cam_project(ProjCam cam, int n, const double *__restrict__ P, double *__restrict__ px) {
  const int k = blockIdx.x * REMAP_PROJECT_THREADS + threadIdx.x;
  if (k >= n) return;
  const CamPixel p = cam_project(cam, P[3 * k], P[3 * k + 1], P[3 * k + 2]);
  px[2 * k] = p.u, px[2 * k + 1] = p.v;
}

struct RemapBuildArgs {  // by value
  ProjCam cam;
  int kind, width, height;
  double M[9];
  RemapGeom g;  // bpp 0: no integer map yet
};

// The bodies of k_remap_build and k_remap_index: the kernels below and their *_b entries (kernels_trackbatch.h: a slot of the batched
// route in blockIdx.z) run them.
DEV void remap_build_body(const RemapBuildArgs &a, float *__restrict__ map_x, float *__restrict__ map_y, int *__restrict__ imap) {
  const int i = blockIdx.x * REMAP_TILE_W + (threadIdx.x % REMAP_TILE_W), j = blockIdx.y * REMAP_TILE_H + (threadIdx.x / REMAP_TILE_W);
  if (i >= a.width || j >= a.height) return;
  const RemapEntry e = remap_entry(a.cam, a.kind, a.width, a.height, a.M, i, j);
  const size_t p = (size_t)j * a.width + i;
  map_x[p] = e.x, map_y[p] = e.y;
  if (a.g.bpp) imap[p] = remap_offset(e.x, e.y, a.g);
}
DEV void remap_index_body(const RemapGeom &g, size_t pixels, const float *__restrict__ map_x, const float *__restrict__ map_y, int *__restrict__ imap) {
  const size_t p = (size_t)blockIdx.x * REMAP_THREADS + threadIdx.x;
  if (p >= pixels) return;
  imap[p] = remap_offset(map_x[p], map_y[p], g);
}

__global__ __launch_bounds__(REMAP_THREADS) void k_remap_build(RemapBuildArgs a, float *__restrict__ map_x, float *__restrict__ map_y, int *__restrict__ imap) {
  remap_build_body(a, map_x, map_y, imap);
}

__global__ __launch_bounds__(REMAP_THREADS) void k_remap_index(RemapGeom g, size_t pixels, const float *__restrict__ map_x, const float *__restrict__ map_y,
                                                               int *__restrict__ imap) {
  remap_index_body(g, pixels, map_x, map_y, imap);
}

template <int BPP>
__global__ __launch_bounds__(REMAP_THREADS) void k_remap_apply(const int *__restrict__ imap, const unsigned char *__restrict__ src, unsigned char *__restrict__ out,
                                                               size_t pixels) {
  const size_t p0 = ((size_t)blockIdx.x * REMAP_THREADS + threadIdx.x) * REMAP_RUN;
  if (p0 >= pixels) return;
  if (p0 + REMAP_RUN <= pixels) {
    const int4 o4 = *(const int4 *)(imap + p0);
    const int off[REMAP_RUN] = {o4.x, o4.y, o4.z, o4.w};
    unsigned w[BPP];
#pragma unroll
    for (int k = 0; k < BPP; k++) w[k] = 0u;
#pragma unroll
    for (int j = 0; j < REMAP_RUN; j++) {
      const unsigned char *s = src + (off[j] < 0 ? 0 : off[j]);
#pragma unroll
      for (int k = 0; k < BPP; k++) {
        const unsigned b = off[j] < 0 ? 0u : (unsigned)s[k];
        w[(j * BPP + k) >> 2] |= b << (((j * BPP + k) & 3) * 8);  // constant indices once unrolled
      }
    }
    unsigned *dst = (unsigned *)(out + p0 * BPP);
#pragma unroll
    for (int k = 0; k < BPP; k++) dst[k] = w[k];
  } else {
    for (size_t p = p0; p < pixels; p++) {
      const int o = imap[p];
      for (int k = 0; k < BPP; k++) out[p * BPP + k] = o < 0 ? (unsigned char)0 : src[o + k];
    }
  }
}

// bpp: 1 .. 4 (imgfmt_bpp of a checked encoding)
inline void remap_apply_launch(hipStream_t fs, int bpp, const int *imap, const unsigned char *src, unsigned char *out, size_t pixels) {
  const dim3 grid(remap_apply_blocks(pixels)), block(REMAP_THREADS);
  switch (bpp) {
    case 1: hipLaunchKernelGGL(k_remap_apply<1>, grid, block, 0, fs, imap, src, out, pixels); break;
    case 2: hipLaunchKernelGGL(k_remap_apply<2>, grid, block, 0, fs, imap, src, out, pixels); break;
    case 3: hipLaunchKernelGGL(k_remap_apply<3>, grid, block, 0, fs, imap, src, out, pixels); break;
    default: hipLaunchKernelGGL(k_remap_apply<4>, grid, block, 0, fs, imap, src, out, pixels); break;
  }
}
