// kernels_imgfmt.h — k_img_gray: a camera image in one of the encodings of image_format.h into 8-bit grey, behind lfvio_image_gray and
// the write of level 0 of the fresh pyramid in lfvio_klt_track / lfvio_track_frame (klt.inc: where the device-to-device copy stands
// without a format) and, with the slot in blockIdx.z, lfvio_track_batch_frame (k_img_gray_b, kernels_trackbatch.h: where k_tb_image
// stands).  The grey value of a pixel is imgfmt_gray of image_format.h, the text the host runs.
//
//   grid (columns / 256, rows / 4), 256 threads: a wave per row, a lane per run of 4 output pixels, so a wave reads 256 * bytes per
//   pixel contiguous bytes of one row and writes 256 contiguous bytes.
//   wide path  the image's first byte, `step`, the output's first byte and `width` are all multiples of 4: the lane's 4 * bytes per
//              pixel input bytes are 1 .. 4 dwords, adjacent in the lane and from lane to lane (the loads merge into one of up to 16
//              bytes per lane), the 4 grey bytes leave as one dword.
//   byte path  anything else: byte loads and byte stores of the same pixels.  Both paths give the same bytes.
//   Neither reads a byte outside a row's first width * bytes per pixel (<= step) bytes: the wide path runs only where width % 4 == 0,
//   so a lane's 4 pixels are all the row's.
#pragma once
#include "dev_math.h"
#include "image_format.h"

constexpr int IMG_THREADS = 256, IMG_COLS = 256, IMG_ROWS = 4;  // of one workgroup: 64 lanes of 4 pixels, 4 rows

template <int BPP>
DEV void img_gray_run(int code, const unsigned char *src, size_t step, unsigned char *dst, int W, int H) {
  const int x0 = blockIdx.x * IMG_COLS + (threadIdx.x & 63) * 4, y = blockIdx.y * IMG_ROWS + (threadIdx.x >> 6);
  if (x0 >= W || y >= H) return;
  const unsigned char *in = src + (size_t)y * step + (size_t)x0 * BPP;
  unsigned char *out = dst + (size_t)y * W + x0;
  if ((((size_t)src | step | (size_t)dst | (size_t)W) & 3) == 0) {  // (uniform over the grid)
    unsigned w[BPP];
#pragma unroll
    for (int k = 0; k < BPP; k++) w[k] = ((const unsigned *)in)[k];
    unsigned o = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      unsigned b[3] = {0, 0, 0};  // the pixel's first min(BPP, 3) bytes: constant indices once unrolled
#pragma unroll
      for (int k = 0; k < (BPP < 3 ? BPP : 3); k++) b[k] = (w[(j * BPP + k) >> 2] >> (((j * BPP + k) & 3) * 8)) & 255u;
      o |= imgfmt_gray(code, b[0], b[1], b[2]) << (8 * j);
    }
    *(unsigned *)out = o;
  } else {
#pragma unroll
    for (int j = 0; j < 4; j++)
      if (x0 + j < W) {
        const unsigned char *p = in + j * BPP;
        out[j] = (unsigned char)imgfmt_gray(code, p[0], BPP > 1 ? p[1] : 0u, BPP > 2 ? p[2] : 0u);
      }
  }
}
// code: one of the table (the host has checked it); step >= W * bytes per pixel
DEV void img_gray_body(int code, const unsigned char *src, size_t step, unsigned char *dst, int W, int H) {
  switch (imgfmt_bpp(code)) {
    case 1: img_gray_run<1>(code, src, step, dst, W, H); break;
    case 2: img_gray_run<2>(code, src, step, dst, W, H); break;
    case 3: img_gray_run<3>(code, src, step, dst, W, H); break;
    case 4: img_gray_run<4>(code, src, step, dst, W, H); break;
    default: break;
  }
}
__global__ __launch_bounds__(IMG_THREADS) void k_img_gray(int code, const unsigned char *src, size_t step, unsigned char *dst, int W, int H) {
  img_gray_body(code, src, step, dst, W, H);
}
