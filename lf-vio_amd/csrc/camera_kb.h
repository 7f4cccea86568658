// camera_kb.h — the KANNALA_BRANDT camera model (LFVIO_CAM_KANNALA_BRANDT, include/lfvio.h): EquidistantCamera::liftProjective
// (camera_model/src/camera_models/EquidistantCamera.cc:428-442) over backprojectSymmetric (:716-818), restated in operations IEEE 754
// defines (+ - * / sqrt floor and comparisons), each rounded on its own: every user compiles this with -ffp-contract=off.  The
// per-pixel functions are host-and-device functions that the kernels and the host compile, as image_format.h's pixel conversions
// are; camera_models.h, which holds the other three models, includes this file, calls kb_lift_pixel from cam_lift and forms the
// once-per-camera constants on the host in track_cam.  It includes nothing from HIP when compiled for the host: tests/test_kb_ref.py
// compiles it with g++ and holds it to tests/kb_ref.py, the numpy text of the same specification, bit for bit, and
// tests/tools/camera_kb_walk.cpp walks it under the CPU sanitizers.
//
// The model: a pixel (px, py) lies at x = inv11 px + inv13, y = inv22 py + inv23 of the normalised plane (:432-433), at the radius
// r = sqrt(x x + y y); theta is the smallest non-negative real root of
//     f(theta) = theta + k2 theta^3 + k3 theta^5 + k4 theta^7 + k5 theta^9 = r,
// and the ray is (sin theta x / r, sin theta y / r, cos theta).
//
// Stated deviations from the reference's text: x / r, y / r in place of cos(atan2(y, x)), sin(atan2(y, x)); Newton's
// method in place of the eigenvalues of the companion matrix; a root BEHIND a dip of f inside [0, pi] is not looked for (none of the
// reference's three calibrations has one), and the pi / 4096 grid can miss a dip of f' narrower than a grid step.
#pragma once
#include <cmath>
#include <cstring>

#if defined(__HIPCC__)
#define KB_HD __host__ __device__ inline
#else
#define KB_HD inline
#endif

constexpr int KB_NEWTON_STEPS = 13;  // measured: 11 steps bring the residual under its bar everywhere on [0, r_lim]; plus two
constexpr int KB_GRID = 4096;

// ---- the polynomial and its derivative, as Horner forms in t = theta theta; k = k2, k3, k4, k5
KB_HD double kb_f(const double *k, double th) {
  const double t = th * th;
  return th * (1.0 + t * (k[0] + t * (k[1] + t * (k[2] + t * k[3]))));
}
KB_HD double kb_fp(const double *k, double th) {
  const double t = th * th;
  return 1.0 + t * (3.0 * k[0] + t * (5.0 * k[1] + t * (7.0 * k[2] + t * (9.0 * k[3]))));
}

// ---- once per camera, on the host.  theta_lim: the last point of the grid j (pi / 4096), j = 0 .. 4096, up to which f' > 0 held at
// every grid point (pi if at all of them: a bearing's angle cannot exceed pi); r_lim = f(theta_lim).  On [0, theta_lim] f increases from
// 0, so for r <= r_lim its only root there is the smallest non-negative real root: the one the reference picks.
struct KbConstants {
  double theta_lim, r_lim;
};
inline KbConstants kb_constants(const double *k) {
  const double step = 3.14159265358979323846 / (double)KB_GRID;
  KbConstants c = {0.0, 0.0};  // f'(0) = 1
  for (int j = 1; j <= KB_GRID; j++) {
    const double th = (double)j * step;
    if (!(kb_fp(k, th) > 0.0)) break;
    c.theta_lim = th;
  }
  c.r_lim = kb_f(k, c.theta_lim);
  return c;
}

// The scan is 4097 polynomial evaluations and track_cam runs on every call: the constants are kept beside the eight numbers they
// were formed from (the single route: one on the context; the batched route: one per slot), and a steady stream pays a memcmp.
struct KbCache {
  bool valid = false;
  double key[8] = {};  // cx, cy, fx, fy, k2 .. k5: the bytes compared, so -0.0 and 0.0 differ and a padding byte never counts
  KbConstants c = {0.0, 0.0};
  const KbConstants &get(const double *now) {
    if (!valid || std::memcmp(key, now, sizeof key) != 0) {
      c = kb_constants(now + 4);
      std::memcpy(key, now, sizeof key);
      valid = true;
    }
    return c;
  }
};

// ---- per pixel
// KB_NEWTON_STEPS Newton steps from min(r, theta_lim), the iterate clamped to [0, theta_lim] after each; r > r_lim or NaN: theta = r,
// the reference's own fallback when it finds no admissible root (:809-812).  Every choice is a select written so that a NaN takes
// the same side everywhere, and the trip count is fixed: nothing diverges within a wave.  With k2 .. k5 all zero the first step
// leaves theta = r exactly (:771-774).
KB_HD double kb_root(const double *k, double theta_lim, double r_lim, double r) {
  double th = r < theta_lim ? r : theta_lim;
  for (int i = 0; i < KB_NEWTON_STEPS; i++) {
    th = th - (kb_f(k, th) - r) / kb_fp(k, th);
    th = th < 0.0 ? 0.0 : th;
    th = th > theta_lim ? theta_lim : th;
  }
  return r <= r_lim ? th : r;
}

// sin and cos of theta >= 0.  n = floor(theta (2 / pi) + 0.5) stays a double, a three-part Cody-Waite subtraction of n pi / 2, the
// quadrant n - 4 floor(n / 4) in double again, and two fixed-degree kernels on [-pi / 4, pi / 4]: nothing that can be NaN, infinite or
// huge is converted to an integer (x86 and gfx950 differ there, and pixels are arbitrary floats).  About 1.3 ulp while n < 2^20 (the
// products n PIO2_1 and n PIO2_2 are exact); beyond that range the result is only the same bits on every side.
// The constants: invpio2, pio2_1, pio2_2, pio2_2t of e_rem_pio2.c and S1 .. S6 of k_sin.c, C1 .. C6 of k_cos.c, fdlibm 5.3 (Sun
// Microsystems, 1993; the text FreeBSD's msun carries) — public, and the minimax coefficients most libms share.
KB_HD void kb_sincos(double th, double &sn, double &cn) {
  constexpr double INVPIO2 = 6.36619772367581382433e-01;
  constexpr double PIO2_1 = 1.57079632673412561417e+00, PIO2_2 = 6.07710050630396597660e-11, PIO2_2T = 2.02226624879595063154e-21;
  constexpr double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03, S3 = -1.98412698298579493134e-04;
  constexpr double S4 = 2.75573137070700676789e-06, S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
  constexpr double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03, C3 = 2.48015872894767294178e-05;
  constexpr double C4 = -2.75573143513906633035e-07, C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
  const double n = floor(th * INVPIO2 + 0.5);
  const double y = ((th - n * PIO2_1) - n * PIO2_2) - n * PIO2_2T;
  const double q = n - 4.0 * floor(n / 4.0);
  const double z = y * y;
  const double s = y + (z * y) * (S1 + z * (S2 + z * (S3 + z * (S4 + z * (S5 + z * S6)))));
  const double c = 1.0 - (0.5 * z - z * (z * (C1 + z * (C2 + z * (C3 + z * (C4 + z * (C5 + z * C6)))))));
  const bool swap = q == 1.0 || q == 3.0;
  const double a = swap ? c : s, b = swap ? s : c;
  sn = (q == 2.0 || q == 3.0) ? -a : a;
  cn = (q == 1.0 || q == 2.0) ? -b : b;
}

// the ray of the point (x, y) of the normalised plane
KB_HD void kb_lift_plane(const double *k, double theta_lim, double r_lim, double x, double y, double &X, double &Y, double &Z) {
  const double r = sqrt(x * x + y * y);
  double sn, cn;
  kb_sincos(kb_root(k, theta_lim, r_lim, r), sn, cn);
  const bool tiny = r < 1e-10;  // :722-725: phi = 0
  const double cphi = tiny ? 1.0 : x / r, sphi = tiny ? 0.0 : y / r;
  X = sn * cphi, Y = sn * sphi, Z = cn;
}

// the ray of the pixel (px, py): the normalised plane (:432-433) with the inverse projection matrix's four entries, then the above
KB_HD void kb_lift_pixel(double inv11, double inv13, double inv22, double inv23, const double *k, double theta_lim, double r_lim, float px,
                         float py, double &X, double &Y, double &Z) {
  const double x = inv11 * (double)px + inv13, y = inv22 * (double)py + inv23;
  kb_lift_plane(k, theta_lim, r_lim, x, y, X, Y, Z);
}
