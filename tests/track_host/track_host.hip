// Host-side driver of the trajectory-tracking law (TEST-ONLY): track_references and desired_accel_track of
// csrc/dat_track.hpp, compiled with hipcc into tests/track_host/libdat_track_host.so and loaded only by tests/.
// They are the functions k_desired, k_advance, k_rp_advance and the logging rollout call, so the law can be checked
// against the reference's recording and the numpy statement without a GPU.
#include "../../distributed_aerial_transportation_amd/csrc/dat_track.hpp"

using namespace dat;

extern "C" {

// x_ref, v_ref, a_ref of `count` records (DAT_TRACK_SIZE doubles each) at the simulation steps tick[k], t = tick dt
void th_references(const double* rec, const long long* tick, double dt, int count, double* xr, double* vr,
                   double* ar) {
  for (int k = 0; k < count; ++k)
    track_references(rec + (size_t)k * DAT_TRACK_SIZE, track_time(tick[k], dt), xr + 3 * k, vr + 3 * k, ar + 3 * k);
}

// acc (6 each) of `count` state blocks (S doubles each) under their records at tick[k]
void th_desired(const double* st, int n, int S, const double* rec, const long long* tick, double dt, int count,
                double* acc) {
  for (int k = 0; k < count; ++k)
    desired_accel_track(st + (size_t)k * S, n, rec + (size_t)k * DAT_TRACK_SIZE, track_time(tick[k], dt), acc + 6 * k);
}

// the forest law on the same blocks (the clamp the tracking law's is held to): flat-ground mountain record
void th_desired_forest(const double* st, int n, int S, const double* mountain, double x_offset, int count,
                       double* acc) {
  for (int k = 0; k < count; ++k) desired_accel_forest(st + (size_t)k * S, n, mountain, x_offset, acc + 6 * k);
}

// first field of a record dat_set_tracking rejects, -1: none
int th_bad_field(const double* rec) { return track_record_bad_field(rec); }

}  // extern "C"
