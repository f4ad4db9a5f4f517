// dat_track.hpp -- the time-dependent trajectory-tracking law of the reference's controller tests
// (test/control/test_rqpcontrollers.py:24-48 _desired_acceleration_noenv, test/control/test_rpcentralized.py:14-38
// _desired_acceleration): a circle flown at constant angular rate with feed-forward acceleration, stated once for the
// kernels (k_desired, k_advance, k_rp_advance, the logging rollout) and the host (tests/track_host).  Every
// floating-point expression stands whole inside one function (the rule of dat_cadmm_step.hpp), so the callers differ
// only in their sin / cos.
//
// The tracking record of a scenario (DAT_TRACK_SIZE doubles, dat_layout.h DAT_T_*): centre, radius, height, angular
// rate FREQ, time offset T0, the gains KP and KV, the clamp AMAX on |dvl_des| (<= 0: none, as the reference), and the
// amplitude and z component of dwl_des.  At time t, with tau = t + T0 and theta = FREQ tau:
//   x_ref = (CX + R cos theta, CY + R sin theta, HEIGHT)
//   v_ref = (-R FREQ sin theta, R FREQ cos theta, 0)
//   a_ref = (-R FREQ^2 cos theta, -R FREQ^2 sin theta, 0)
//   dvl_des = a_ref - KV (vl - v_ref) - KP (xl - x_ref), clamped to AMAX as the forest law clamps to 1
//   dwl_des = (WAMP sin tau, WAMP cos tau, WZ)
#pragma once

#include "dat_core.hpp"

namespace dat {

// the law's time at simulation step `tick` (the reference's t_seq[i] = np.arange(0, T, dt)[i] is i * dt to the bit)
DAT_HD double track_time(long long tick, double dt) { return (double)tick * dt; }

// x_ref, v_ref, a_ref at time t
DAT_HD void track_references(const double* rec, double t, double* xr, double* vr, double* ar) {
  const double tau = t + rec[DAT_T_T0];
  const double th = rec[DAT_T_FREQ] * tau;
  const double c = cos(th), s = sin(th);
  const double R = rec[DAT_T_RADIUS], w = rec[DAT_T_FREQ];
  xr[0] = rec[DAT_T_CX] + R * c;
  xr[1] = rec[DAT_T_CY] + R * s;
  xr[2] = rec[DAT_T_HEIGHT];
  vr[0] = -R * w * s;
  vr[1] = R * w * c;
  vr[2] = 0.0;
  ar[0] = -R * (w * w) * c;
  ar[1] = -R * (w * w) * s;
  ar[2] = 0.0;
}

// acc = (dvl_des, dwl_des) from the payload's position and velocity
DAT_HD void desired_accel_track_at(const double* xl, const double* vl, const double* rec, double t, double* acc) {
  double xr[3], vr[3], ar[3];
  track_references(rec, t, xr, vr, ar);
  const double kp = rec[DAT_T_KP], kv = rec[DAT_T_KV];
  double d[3];
  for (int c = 0; c < 3; ++c) {
    const double ev = kv * (vl[c] - vr[c]);
    const double ex = kp * (xl[c] - xr[c]);
    d[c] = ar[c] - ev - ex;
  }
  const double amax = rec[DAT_T_AMAX];
  if (amax > 0.0) {  // the forest law's clamp (desired_accel_forest), to AMAX instead of 1
    double dn = sqrt(dot3(d, d));
    if (dn > 0) {
      double s = fmin(dn, amax) / dn;
      for (int c = 0; c < 3; ++c) d[c] *= s;
    }
  }
  const double tau = t + rec[DAT_T_T0];
  acc[0] = d[0]; acc[1] = d[1]; acc[2] = d[2];
  acc[3] = rec[DAT_T_WAMP] * sin(tau);
  acc[4] = rec[DAT_T_WAMP] * cos(tau);
  acc[5] = rec[DAT_T_WZ];
}

// ... from a state block (the form of desired_accel_forest)
DAT_HD void desired_accel_track(const double* st, int n, const double* rec, double t, double* acc) {
  desired_accel_track_at(st + DAT_S_XL(n), st + DAT_S_VL(n), rec, t, acc);
}

// A record the law accepts: every field finite, RADIUS, FREQ, KP, KV >= 0 (host side: dat_set_tracking).  Returns the
// index of the first offending field, -1: none.
inline int track_record_bad_field(const double* rec) {
  for (int k = 0; k < DAT_TRACK_SIZE; ++k)
    if (!(rec[k] - rec[k] == 0.0)) return k;
  const int nonneg[4] = {DAT_T_RADIUS, DAT_T_FREQ, DAT_T_KP, DAT_T_KV};
  for (int k : nonneg)
    if (rec[k] < 0.0) return k;
  return -1;
}

}  // namespace dat
