// kernels_tracksource.h — k_remap_gray: level 0 of the fresh pyramid gathered from the SOURCE image through the resident integer map,
// behind lfvio_track_source_set (include/lfvio.h; host side: tracksource.inc).  It stands where k_remap_apply, a copy
// down, a copy up and k_img_gray stood: the grey value of a pixel is imgfmt_gray (image_format.h) of the bytes k_remap_apply
// (kernels_remap.h) would have written, the text the host runs too (tracksource_lane, tracksource_plan.h).
//
//   k_remap_apply's geometry: the output is one run of W * H pixels and a lane takes REMAP_RUN = 4 consecutive ones — one 16-byte load
//   of the integer map, per pixel min(BPP, 3) byte loads from the source (a fourth byte is never read into a grey value), imgfmt_gray
//   per pixel, ONE dword stored into level 0; the run's last fewer-than-4 pixels go byte by byte.  An outside entry still loads — byte
//   0 .. of the source, which every source has — and selects zero, so no load hangs on a branch; its grey value is that of a zero
//   pixel.  `code` and BPP are the same for the whole grid.  Per output pixel 4 + BPP + 1 bytes move, against (4 + 2 BPP) + (BPP + 1)
//   of the two kernels it replaces.
//   Bounds: kernels_remap.h's — an offset is sy * step + sx * BPP with sx < sw, sy < sh, step >= sw * BPP, so offset + BPP <= sh * step,
//   the bytes uploaded; lanes past the last pixel return before any access; level 0 and the integer map start allocations aligned to
//   256 bytes, so the dword store and the int4 load are aligned for every W; the source is read by bytes, so neither its place in the
//   staging block nor its step needs an alignment.
#pragma once
#include "dev_math.h"
#include "image_format.h"
#include "remap_plan.h"

// The body: k_remap_gray below and k_remap_gray_b (kernels_trackbatch.h: a slot of the batched route in blockIdx.z) run it.
template <int BPP>
DEV void remap_gray_body(int code, const int *__restrict__ imap, const unsigned char *__restrict__ src, unsigned char *__restrict__ level0, size_t pixels) {
  constexpr int NB = BPP < 3 ? BPP : 3;
  const size_t p0 = ((size_t)blockIdx.x * REMAP_THREADS + threadIdx.x) * REMAP_RUN;
  if (p0 >= pixels) return;
  if (p0 + REMAP_RUN <= pixels) {
    const int4 o4 = *(const int4 *)(imap + p0);
    const int off[REMAP_RUN] = {o4.x, o4.y, o4.z, o4.w};
    unsigned w = 0u;
#pragma unroll
    for (int j = 0; j < REMAP_RUN; j++) {
      const unsigned char *s = src + (off[j] < 0 ? 0 : off[j]);
      unsigned b[3] = {0u, 0u, 0u};  // constant indices once unrolled
#pragma unroll
      for (int k = 0; k < NB; k++) b[k] = off[j] < 0 ? 0u : (unsigned)s[k];
      w |= imgfmt_gray(code, b[0], b[1], b[2]) << (8 * j);
    }
    *(unsigned *)(level0 + p0) = w;
  } else {
    for (size_t p = p0; p < pixels; p++) {
      const int o = imap[p];
      const unsigned char *s = src + (o < 0 ? 0 : o);
      unsigned b[3] = {0u, 0u, 0u};
#pragma unroll
      for (int k = 0; k < NB; k++) b[k] = o < 0 ? 0u : (unsigned)s[k];
      level0[p] = (unsigned char)imgfmt_gray(code, b[0], b[1], b[2]);
    }
  }
}
template <int BPP>
__global__ __launch_bounds__(REMAP_THREADS) void k_remap_gray(int code, const int *__restrict__ imap, const unsigned char *__restrict__ src,
                                                              unsigned char *__restrict__ level0, size_t pixels) {
  remap_gray_body<BPP>(code, imap, src, level0, pixels);
}

// code: one of image_format.h's table (the host has checked it); imap: written for this source's geometry
inline void remap_gray_launch(hipStream_t fs, int code, const int *imap, const unsigned char *src, unsigned char *level0, size_t pixels) {
  const dim3 grid(remap_apply_blocks(pixels)), block(REMAP_THREADS);
  switch (imgfmt_bpp(code)) {
    case 1: hipLaunchKernelGGL(k_remap_gray<1>, grid, block, 0, fs, code, imap, src, level0, pixels); break;
    case 2: hipLaunchKernelGGL(k_remap_gray<2>, grid, block, 0, fs, code, imap, src, level0, pixels); break;
    case 3: hipLaunchKernelGGL(k_remap_gray<3>, grid, block, 0, fs, code, imap, src, level0, pixels); break;
    default: hipLaunchKernelGGL(k_remap_gray<4>, grid, block, 0, fs, code, imap, src, level0, pixels); break;
  }
}
