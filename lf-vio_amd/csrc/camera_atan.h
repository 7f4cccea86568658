// camera_atan.h — the arctangent that the projections of camera_models.h take (cam_project: OCam's elevation angle, KANNALA_BRANDT's
// theta), in operations IEEE 754 defines (+ - * /, comparisons and fabs), each rounded on its own: every user compiles this with
// -ffp-contract=off, and numpy (tests/project_ref.py) and the device share its bits.  Plain C++ without hipcc; a host-and-device
// function under it (KB_HD of camera_kb.h).  No libm call and no builtin.
//
// The scheme is s_atan.c's of fdlibm 5.3 (Sun Microsystems, 1993; the text FreeBSD's msun carries — public): |x| is reduced on four
// intervals to t with atan|x| = atanhi + atanlo + atan(t),
//     [7/16, 11/16)   (2|x| - 1) / (2 + |x|)    atan(0.5)
//     [11/16, 19/16)  (|x| - 1) / (|x| + 1)     atan(1)
//     [19/16, 39/16)  (|x| - 1.5) / (1 + 1.5|x|) atan(1.5)
//     [39/16, inf]    -1 / |x|                  atan(inf) = pi / 2
// below 7/16 t = |x|; atan(t) = t - t (s1 + s2) with the eleven coefficients aT[0 .. 10] split into the odd and the even powers of
// z = t t.  fdlibm compares the high word; its thresholds have a zero low word, so comparing the doubles is the same test.  Every
// choice is a select: one division per call and nothing diverges within a wave.  |x| < 2^-29 returns x itself (-0.0 stays -0.0),
// |x| >= 2^66 returns +-(atanhi[3] + atanlo[3]), a NaN falls through every comparison and comes out of the polynomial as a NaN.
// tests/test_project_ref.py holds the numpy text to 50 digits; tests/test_camera_project.py holds this file to the numpy text.
#pragma once
#include <cmath>

#include "camera_kb.h"

KB_HD double cam_atan(double x) {
  constexpr double HI0 = 4.63647609000806093515e-01, HI1 = 7.85398163397448278999e-01, HI2 = 9.82793723247329054082e-01,
                   HI3 = 1.57079632679489655800e+00;
  constexpr double LO0 = 2.26987774529616870924e-17, LO1 = 3.06161699786838301793e-17, LO2 = 1.39033110312309984516e-17,
                   LO3 = 6.12323399573676603587e-17;
  constexpr double A0 = 3.33333333333329318027e-01, A1 = -1.99999999998764832476e-01, A2 = 1.42857142725034663711e-01;
  constexpr double A3 = -1.11111104054623557880e-01, A4 = 9.09088713343650656196e-02, A5 = -7.69187620504482999495e-02;
  constexpr double A6 = 6.66107313738753120669e-02, A7 = -5.83357013379057348645e-02, A8 = 4.97687799461593236017e-02;
  constexpr double A9 = -3.65315727442169155270e-02, A10 = 1.62858201153657823623e-02;
  constexpr double TINY = 3.7252902984619140625e-09 /* 2^-29 */, HUGE_ = 73786976294838206464.0 /* 2^66 */;
  const double a = fabs(x);
  const bool i0 = a >= 0.4375, i1 = a >= 0.6875, i2 = a >= 1.1875, i3 = a >= 2.4375;
  const double num = i3 ? -1.0 : i2 ? a - 1.5 : i1 ? a - 1.0 : i0 ? 2.0 * a - 1.0 : a;
  const double den = i3 ? a : i2 ? 1.0 + 1.5 * a : i1 ? a + 1.0 : i0 ? 2.0 + a : 1.0;
  const double hi = i3 ? HI3 : i2 ? HI2 : i1 ? HI1 : HI0, lo = i3 ? LO3 : i2 ? LO2 : i1 ? LO1 : LO0;
  const double t = num / den;
  const double z = t * t, w = z * z;
  const double s1 = z * (A0 + w * (A2 + w * (A4 + w * (A6 + w * (A8 + w * A10)))));
  const double s2 = w * (A1 + w * (A3 + w * (A5 + w * (A7 + w * A9))));
  const double ts = t * (s1 + s2);
  double r = i0 ? hi - ((ts - lo) - t) : t - ts;
  r = a >= HUGE_ ? HI3 + LO3 : r;
  r = x < 0.0 ? -r : r;
  return a < TINY ? x : r;
}
