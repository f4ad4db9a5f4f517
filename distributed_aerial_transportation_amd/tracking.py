"""The reference's trajectory-tracking law in numpy, and the records that select it on the device.

The reference's controllers fly a time-dependent law when there is no forest (test/control/test_rqpcontrollers.py:24-48
``_desired_acceleration_noenv``, test/control/test_rpcentralized.py:14-38): a circle of radius 1 m at 1 m height,
0.5 rad/s, with feed-forward ``a_ref``, no clamp, and ``dwl_des = (sin t, cos t, pi / 12)``.  The device states it in
``csrc/dat_track.hpp``; a scenario's tracking record (``layout.TRACK_SIZE`` doubles, fields ``layout.T``) generalises
it to a circle family.  With tau = t + T0 and theta = FREQ tau:

    x_ref = (CX + R cos theta, CY + R sin theta, HEIGHT)
    v_ref = (-R FREQ sin theta, R FREQ cos theta, 0)
    a_ref = (-R FREQ^2 cos theta, -R FREQ^2 sin theta, 0)
    dvl_des = a_ref - KV (vl - v_ref) - KP (xl - x_ref), clamped to AMAX (> 0) as the forest law clamps to 1
    dwl_des = (WAMP sin tau, WAMP cos tau, WZ)

``BatchedController.set_tracking(records)`` selects the law on the device; ``references`` and ``desired_acceleration``
are the numpy statement the tests and ``example`` use.  On the reference's record the statement evaluates the
reference's own expressions, operation for operation.
"""

from __future__ import annotations

import numpy as np

from . import layout

T = layout.T
TRACK_SIZE = layout.TRACK_SIZE


def circle_record(center=(0.0, 0.0), radius: float = 1.0, height: float = 1.0, freq: float = 0.5, t0: float = 0.0,
                  kp: float = 1.0, kv: float = 1.0, amax: float = 0.0, wamp: float = 1.0,
                  wz: float = np.pi / 12) -> np.ndarray:
    """One tracking record; the defaults are the reference's circle (amax <= 0: no clamp)."""
    r = np.zeros(TRACK_SIZE)
    r[T["CX"]], r[T["CY"]] = center
    r[T["RADIUS"]], r[T["HEIGHT"]], r[T["FREQ"]], r[T["T0"]] = radius, height, freq, t0
    r[T["KP"]], r[T["KV"]], r[T["AMAX"]], r[T["WAMP"]], r[T["WZ"]] = kp, kv, amax, wamp, wz
    return r


def _fields(rec):
    rec = np.asarray(rec, float)
    return [rec[..., T[k]] for k in ("CX", "CY", "RADIUS", "HEIGHT", "FREQ", "T0", "KP", "KV", "AMAX", "WAMP", "WZ")]


def references(rec, t):
    """(x_ref, v_ref, a_ref) at time t: rec (TRACK_SIZE,) or (B, TRACK_SIZE), t a scalar or (B,); (..., 3) each."""
    cx, cy, radius, height, freq, t0, *_ = _fields(rec)
    tau = t + t0
    c, s = np.cos(freq * tau), np.sin(freq * tau)
    zero = np.zeros_like(c)
    x_ref = np.stack([cx + radius * c, cy + radius * s, height + zero], axis=-1)
    v_ref = np.stack([-radius * freq * s, radius * freq * c, zero], axis=-1)
    a_ref = np.stack([-radius * freq ** 2 * c, -radius * freq ** 2 * s, zero], axis=-1)
    return x_ref, v_ref, a_ref


def desired_acceleration(xl, vl, rec, t) -> np.ndarray:
    """acc = (dvl_des, dwl_des), (..., 6), from the payload's position xl and velocity vl (..., 3)."""
    _, _, _, _, _, t0, kp, kv, amax, wamp, wz = _fields(rec)
    x_ref, v_ref, a_ref = references(rec, t)
    xl, vl = np.asarray(xl, float), np.asarray(vl, float)
    d = a_ref - np.asarray(kv)[..., None] * (vl - v_ref) - np.asarray(kp)[..., None] * (xl - x_ref)
    dn = np.sqrt(np.sum(d * d, axis=-1))
    clamp = (np.asarray(amax) > 0) & (dn > 0)
    scale = np.where(clamp, np.minimum(dn, amax) / np.where(dn > 0, dn, 1.0), 1.0)
    d = np.where(clamp[..., None], d * scale[..., None], d)
    tau = t + t0
    dw = np.stack([wamp * np.sin(tau), wamp * np.cos(tau), wz + np.zeros_like(tau)], axis=-1)
    return np.concatenate([d, dw], axis=-1)


__all__ = ["TRACK_SIZE", "circle_record", "references", "desired_acceleration"]
