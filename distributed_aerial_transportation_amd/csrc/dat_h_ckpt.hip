// dat_h_ckpt.hip -- the checkpoints on the host side (include/dat.h, dat_checkpoint_*): the argument checks of
// dat_ckpt.hpp, the staging buffer and the index lists, the copies and their spans.  No kernel lives here: the
// gather / scatter kernels are dat_k_step.hip's; the record's arguments (ck_args) are dat_handle.hpp's, shared with
// the episodes' respawn.
#include "dat_handle.hpp"

namespace {
// the spans of a save / load (events of the handle's, recorded on its stream and reached): its kernel, its host copy
int ck_times(dat_handle* h, hipEvent_t k0, hipEvent_t k1, hipEvent_t c0, hipEvent_t c1) {
  float km = 0.f, cm = 0.f;
  HIPCHK(hipEventElapsedTime(&km, k0, k1));
  HIPCHK(hipEventElapsedTime(&cm, c0, c1));
  h->ck_kernel_ms = km;
  h->ck_copy_ms = cm;
  return 0;
}
}  // namespace

extern "C" {

int dat_checkpoint_bytes(dat_handle* h, int count, long long* bytes) {
  if (!h || !bytes) return fail("dat_checkpoint_bytes: null argument");
  if (count < 0) return fail("dat_checkpoint_bytes: negative count " + std::to_string(count));
  *bytes = ck_blob_bytes(h->cfg.mode, h->cfg.n, count);
  return 0;
}

int dat_checkpoint_save(dat_handle* h, const int* scenarios, int count, void* blob, long long bytes) {
  if (!h) return fail("dat_checkpoint_save: null handle");
  std::string m;
  if (ck_check_save(h->cfg.mode, h->cfg.n, h->cfg.batch, scenarios, count, blob, bytes, &m)) return fail(m);
  HIPCHK(hipSetDevice(h->cfg.device));
  for (hipStream_t s : h->streams) HIPCHK(hipStreamSynchronize(s));
  ck_put_header(blob, h->cfg.mode, h->cfg.n, count);
  if (count == 0) return 0;
  const dat::CkArgs c = ck_args(h);
  const size_t words = (size_t)count * c.words;
  if (ck_grow(h, &h->ck_stage, &h->ck_stage_cap, words)) return -1;
  if (scenarios) {
    if (ck_grow(h, &h->ck_list, &h->ck_list_cap, (size_t)count)) return -1;
    HIPCHK(hipMemcpyAsync(h->ck_list, scenarios, sizeof(int) * count, hipMemcpyHostToDevice, h->stream));
  }
  const int* list = scenarios ? h->ck_list : nullptr;
  HIPCHK(hipEventRecord(h->e0, h->stream));
  HIPCHK(launch_k_ckpt_gather(ck_wide(c), h->stream, c, list, count, h->ck_stage));
  HIPCHK(hipEventRecord(h->ek, h->stream));
  HIPCHK(hipMemcpyAsync((char*)blob + DAT_CK_HEADER_BYTES, h->ck_stage, sizeof(double) * words, hipMemcpyDeviceToHost,
                        h->stream));
  HIPCHK(hipEventRecord(h->e1, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return ck_times(h, h->e0, h->ek, h->ek, h->e1);
}

int dat_checkpoint_load(dat_handle* h, const void* blob, long long bytes, const int* records, const int* scenarios,
                        int count) {
  if (!h) return fail("dat_checkpoint_load: null handle");
  if (admit(h, "dat_checkpoint_load", ACT_CKPT_LOAD)) return -1;  // (nothing was written)
  std::string m;
  long long lo = 0, hi = 0;
  if (ck_check_load(h->cfg.mode, h->cfg.n, h->cfg.batch, blob, bytes, records, scenarios, count, &lo, &hi, &m))
    return fail(m);
  if (count == 0) return 0;
  HIPCHK(hipSetDevice(h->cfg.device));
  for (hipStream_t s : h->streams) HIPCHK(hipStreamSynchronize(s));
  const dat::CkArgs c = ck_args(h);
  // the records named lie in [lo, hi) of the blob: that stretch is uploaded, once
  const size_t words = (size_t)(hi - lo) * c.words;
  if (ck_grow(h, &h->ck_stage, &h->ck_stage_cap, words) || ck_grow(h, &h->ck_list, &h->ck_list_cap, (size_t)2 * count))
    return -1;
  const hipStream_t st = h->stream;
  HIPCHK(hipEventRecord(h->e0, st));
  HIPCHK(hipMemcpyAsync(h->ck_stage, (const char*)blob + DAT_CK_HEADER_BYTES + sizeof(double) * (size_t)lo * c.words,
                        sizeof(double) * words, hipMemcpyHostToDevice, st));
  int *recs = nullptr, *scen = nullptr;
  if (records) {
    recs = h->ck_list;
    HIPCHK(hipMemcpyAsync(recs, records, sizeof(int) * count, hipMemcpyHostToDevice, st));
  }
  if (scenarios) {
    scen = h->ck_list + count;
    HIPCHK(hipMemcpyAsync(scen, scenarios, sizeof(int) * count, hipMemcpyHostToDevice, st));
  }
  HIPCHK(hipEventRecord(h->ek, st));
  HIPCHK(launch_k_ckpt_scatter(ck_wide(c), st, c, (const double*)h->ck_stage, (const int*)recs, (const int*)scen,
                               (int)lo, count));
  HIPCHK(hipEventRecord(h->e1, st));
  HIPCHK(hipStreamSynchronize(st));
  return ck_times(h, h->ek, h->e1, h->e0, h->ek);
}

int dat_get_checkpoint_ms(dat_handle* h, double* kernel_ms, double* copy_ms) {
  if (!h) return fail("dat_get_checkpoint_ms: null handle");
  if (kernel_ms) *kernel_ms = h->ck_kernel_ms;
  if (copy_ms) *copy_ms = h->ck_copy_ms;
  return 0;
}

}  // extern "C"
