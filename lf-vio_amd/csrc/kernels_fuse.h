// kernels_fuse.h — the kernels behind lfvio_cloud_fuse (include/lfvio.h).  The arithmetic of a point is fuse_point
// (fuse_plan.h), the text the host compiles too; the target's kind, the camera's model and the cloud's layout are kernel arguments, so
// every branch on them is uniform.  A lane per point, 256-thread workgroups, no LDS.
//
//   k_fuse_project   the point's three fields — whole-dword loads when point_step and the offsets are multiples of 4, byte assembly
//                    otherwise —, fuse_point, index[k] written, and for a kept point one atomicMin of (float)r's bit pattern on its pixel
//                    of the range image (filled with +inf's bits before; positive floats order as their bits, so the order of arrival
//                    does not show).  The three counts are a ballot per wave and at most three atomic adds by its first lane.
//   k_fuse_sample    colour[k] = the image's bytes at index[k], zero bytes for -1.
//   k_fuse_paint     the paint's bytes at index[k], byte stores.  Every writer of a pixel writes the same bytes.  It is a launch of
//                    its own BEHIND k_fuse_sample in stream order: one kernel would let a point sample a pixel another has painted.
//   Collisions are rare — 131 072 points into 460 800 pixels — and nothing measured asks for more than this, so
//   nothing is tuned.
//   Bounds: a lane past the last point touches nothing (it takes part in the ballots with a zero vote).  A point's bytes are
//   cloud[k * step + off .. + 4) with off <= step - 4, inside the n * step bytes uploaded; the cloud starts at a 256-aligned offset, so a
//   dword load at a multiple of 4 is aligned.  An index is -1 or row * width + col with col < width, row < height (fuse_point), inside the
//   width * height pixels of range and image; k_fuse_project tests it once more before the atomic.
#pragma once
#include "dev_math.h"
#include "fuse_plan.h"

__global__ __launch_bounds__(FUSE_THREADS) void k_fuse_project(FuseView a, FuseLayout l, int n, const unsigned char *__restrict__ cloud, int *__restrict__ index,
                                                               unsigned *__restrict__ range, int *__restrict__ counts) {
  const int k = blockIdx.x * FUSE_THREADS + threadIdx.x;
  int why = -1;
  if (k < n) {
    const FuseXYZ p = fuse_read(l, cloud, (size_t)k);
    const FuseHit h = fuse_point(a, p.x, p.y, p.z);
    index[k] = h.index;
    why = h.why;
    if (range && h.index >= 0 && h.index < a.width * a.height) atomicMin(range + h.index, __float_as_uint(h.range));
  }
  const unsigned long long kept = __ballot(why == FUSE_KEPT), gate = __ballot(why == FUSE_GATE), proj = __ballot(why == FUSE_PROJECTION);
  if ((threadIdx.x & (warpSize - 1)) == 0) {
    if (kept) atomicAdd(counts + FUSE_KEPT, __popcll(kept));
    if (gate) atomicAdd(counts + FUSE_GATE, __popcll(gate));
    if (proj) atomicAdd(counts + FUSE_PROJECTION, __popcll(proj));
  }
}

__global__ __launch_bounds__(FUSE_THREADS) void k_fuse_sample(int n, int bpp, const int *__restrict__ index, const unsigned char *__restrict__ image,
                                                              unsigned char *__restrict__ colour) {
  const int k = blockIdx.x * FUSE_THREADS + threadIdx.x;
  if (k >= n) return;
  const int p = index[k];
  for (int b = 0; b < bpp; b++) colour[(size_t)k * bpp + b] = p < 0 ? (unsigned char)0 : image[(size_t)p * bpp + b];
}

// paint: the bytes of LfvioFuseIn::paint, the first in the low byte
__global__ __launch_bounds__(FUSE_THREADS) void k_fuse_paint(int n, int bpp, unsigned paint, const int *__restrict__ index, unsigned char *__restrict__ image) {
  const int k = blockIdx.x * FUSE_THREADS + threadIdx.x;
  if (k >= n) return;
  const int p = index[k];
  if (p < 0) return;
  for (int b = 0; b < bpp; b++) image[(size_t)p * bpp + b] = (unsigned char)(paint >> (8 * b));
}
