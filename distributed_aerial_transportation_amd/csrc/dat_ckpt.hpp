// dat_ckpt.hpp -- the checkpoint record's field table and the host-side check of a checkpoint blob
// (dat_checkpoint_save / dat_checkpoint_load, include/dat.h; record and header layout: dat_layout.h, DAT_CK_*).
// Host code only, no HIP: dat.hip includes it, and tests/ckpt_host/ckpt_check_main.cpp compiles it alone.
#pragma once

#include <climits>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/dat.h"
#include "dat_layout.h"

namespace dat {

// ---- the table ---------------------------------------------------------------------------------------------
// Per mode, X(array of dat_handle, words per scenario, record offset): the fp64 arrays of a record, each
// scenario-major in the handle.  The gather and scatter kernels' arguments (dat.hip: ck_args) and the checks below
// are written from these lists and from nothing else.
#define DAT_CK_FIELDS_ALL(X, n)                  \
  X(state, DAT_STATE_SIZE(n), DAT_CK_STATE(n))   \
  X(fdes, 3 * (n), DAT_CK_FDES(n))
#define DAT_CK_FIELDS_CADMM(X, n)                \
  X(cf, 3 * (n) * (n), DAT_CK_F(n))              \
  X(cfbar, 3 * (n), DAT_CK_FMEAN(n))             \
  X(clam, 3 * (n) * (n), DAT_CK_LAMF(n))
#define DAT_CK_FIELDS_DD(X, n)                   \
  X(dlamF, 3 * (n), DAT_CK_LAMF_DD(n))           \
  X(dlamM, 3 * (n), DAT_CK_LAMM_DD(n))           \
  X(dprev, 9 * (n), DAT_CK_PREV_DD(n))
#define DAT_CK_FIELDS_CENT(X, n) X(pf, 3 * (n), DAT_CK_PREVF(n))
// X(int array of dat_handle, index among the ints at DAT_CK_INTS(n)); an array the mode does not have reads as 0
#define DAT_CK_INT_FIELDS(X) X(counter, 0) X(iters, 1) X(ipmx, 2)
// The mode's part of the table: DAT_CK_FIELDS_OF(mode, X, n) expands the lists of `mode` (a run-time value)
#define DAT_CK_FIELDS_OF(mode, X, n)                      \
  do {                                                    \
    DAT_CK_FIELDS_ALL(X, n)                               \
    if ((mode) == DAT_MODE_CADMM) {                       \
      DAT_CK_FIELDS_CADMM(X, n)                           \
    } else if ((mode) == DAT_MODE_DD) {                   \
      DAT_CK_FIELDS_DD(X, n)                              \
    } else {                                              \
      DAT_CK_FIELDS_CENT(X, n)                            \
    }                                                     \
  } while (0)

constexpr int CK_MAX_FIELDS = 5;  // fp64 arrays of one mode's record
constexpr int CK_NINTS = 3;
constexpr int CK_INT_WORDS = 2;   // the ints' words (CK_NINTS ints and a zero, two per word)

inline int ck_record_words(int mode, int n) {
  return mode == DAT_MODE_CADMM ? DAT_CK_WORDS_CADMM(n) : mode == DAT_MODE_DD ? DAT_CK_WORDS_DD(n) : DAT_CK_WORDS_CENT(n);
}
inline long long ck_blob_bytes(int mode, int n, long long count) {
  return DAT_CK_HEADER_BYTES + count * ck_record_words(mode, n) * 8;
}

// the table by name, for messages and for the check that it tiles the record
struct CkField {
  const char* name;
  int words, off;
};
inline int ck_fields(int mode, int n, CkField* f) {
  int k = 0;
#define DAT_CK_X(arr, w, o) f[k++] = CkField{#arr, (w), (o)};
  DAT_CK_FIELDS_OF(mode, DAT_CK_X, n);
#undef DAT_CK_X
  return k;
}
// Do the mode's arrays and the ints cover the record's words once each, up to at most one word of padding?
inline bool ck_table_tiles(int mode, int n) {
  CkField f[CK_MAX_FIELDS + 1];
  int nf = ck_fields(mode, n, f);
  f[nf++] = CkField{"ints", CK_INT_WORDS, DAT_CK_INTS(n)};
  const int words = ck_record_words(mode, n);
  std::vector<int> hit((size_t)words, 0);
  for (int k = 0; k < nf; ++k)
    for (int w = 0; w < f[k].words; ++w) {
      if (f[k].off + w < 0 || f[k].off + w >= words) return false;
      ++hit[(size_t)(f[k].off + w)];
    }
  int holes = 0;
  for (int w = 0; w < words; ++w) {
    if (hit[(size_t)w] > 1) return false;
    if (hit[(size_t)w] == 0 && (++holes > 1 || w != words - 1)) return false;
  }
  return words % 2 == 0;
}

// ---- the header ----------------------------------------------------------------------------------------------
struct CkHeader {
  unsigned long long magic;
  int version, mode, n, words;
  long long count;
};
inline void ck_put_header(void* blob, int mode, int n, long long count) {
  unsigned char* b = (unsigned char*)blob;
  memset(b, 0, DAT_CK_HEADER_BYTES);
  const unsigned long long magic = DAT_CK_MAGIC;
  const int version = DAT_CK_VERSION, words = ck_record_words(mode, n);
  memcpy(b + DAT_CK_H_MAGIC, &magic, 8);
  memcpy(b + DAT_CK_H_VERSION, &version, 4);
  memcpy(b + DAT_CK_H_MODE, &mode, 4);
  memcpy(b + DAT_CK_H_N, &n, 4);
  memcpy(b + DAT_CK_H_WORDS, &words, 4);
  memcpy(b + DAT_CK_H_COUNT, &count, 8);
}

inline int ck_fail(std::string* msg, const std::string& m) {
  if (msg) *msg = m;
  return -1;
}
inline const char* ck_mode_name(int mode) {
  return mode == DAT_MODE_CADMM ? "C-ADMM" : mode == DAT_MODE_DD ? "DD" : mode == DAT_MODE_CENTRALIZED ? "centralized" : "unknown";
}

// ---- the checks: pure functions of their arguments, run before anything is launched or copied --------------------
// The blob against a handle of (mode, n): the header's fields, then `bytes` against the header's record count.
// The blob is outside input: nothing of it is trusted, and nothing past `bytes` is read.
inline int ck_check_header(int mode, int n, const void* blob, long long bytes, CkHeader* out, std::string* msg) {
  const std::string who = "checkpoint blob: ";
  if (!blob) return ck_fail(msg, who + "null pointer");
  if (bytes < DAT_CK_HEADER_BYTES)
    return ck_fail(msg, who + std::to_string(bytes) + " bytes are shorter than the header (" +
                            std::to_string(DAT_CK_HEADER_BYTES) + " bytes)");
  const unsigned char* b = (const unsigned char*)blob;
  CkHeader h;
  memcpy(&h.magic, b + DAT_CK_H_MAGIC, 8);
  memcpy(&h.version, b + DAT_CK_H_VERSION, 4);
  memcpy(&h.mode, b + DAT_CK_H_MODE, 4);
  memcpy(&h.n, b + DAT_CK_H_N, 4);
  memcpy(&h.words, b + DAT_CK_H_WORDS, 4);
  memcpy(&h.count, b + DAT_CK_H_COUNT, 8);
  if (h.magic != (unsigned long long)DAT_CK_MAGIC) return ck_fail(msg, who + "bad magic (not a checkpoint)");
  if (h.version != DAT_CK_VERSION)
    return ck_fail(msg, who + "format version " + std::to_string(h.version) + ", this library reads version " +
                            std::to_string(DAT_CK_VERSION));
  if (h.mode != mode)
    return ck_fail(msg, who + "mode " + std::to_string(h.mode) + " (" + ck_mode_name(h.mode) + "), the handle's mode is " +
                            std::to_string(mode) + " (" + ck_mode_name(mode) + ")");
  if (h.n != n) return ck_fail(msg, who + "n = " + std::to_string(h.n) + ", the handle's n is " + std::to_string(n));
  const int words = ck_record_words(mode, n);
  if (h.words != words)
    return ck_fail(msg, who + std::to_string(h.words) + " words per record, the handle's record has " + std::to_string(words));
  for (int k = DAT_CK_H_PAD; k < DAT_CK_HEADER_BYTES; ++k)
    if (b[k] != 0) return ck_fail(msg, who + "header padding is not zero");
  if (h.count < 0 || h.count > (LLONG_MAX - DAT_CK_HEADER_BYTES) / ((long long)words * 8))
    return ck_fail(msg, who + "record count " + std::to_string(h.count) + " out of range");
  const long long need = ck_blob_bytes(mode, n, h.count);
  if (bytes != need)
    return ck_fail(msg, who + std::to_string(bytes) + " bytes, the header's " + std::to_string(h.count) +
                            " records take " + std::to_string(need));
  if (out) *out = h;
  return 0;
}

// dat_checkpoint_save's arguments against a handle of `batch` scenarios
inline int ck_check_save(int mode, int n, int batch, const int* scenarios, int count, const void* blob, long long bytes,
                         std::string* msg) {
  const std::string who = "dat_checkpoint_save: ";
  if (count < 0) return ck_fail(msg, who + "negative count " + std::to_string(count));
  if (!blob) return ck_fail(msg, who + "null blob");
  if (!scenarios && count != batch)
    return ck_fail(msg, who + "scenarios = NULL means all: count must be the batch " + std::to_string(batch) + ", not " +
                            std::to_string(count));
  for (int k = 0; scenarios && k < count; ++k)
    if (scenarios[k] < 0 || scenarios[k] >= batch)
      return ck_fail(msg, who + "scenario " + std::to_string(scenarios[k]) + " (entry " + std::to_string(k) +
                              ") out of range [0, " + std::to_string(batch) + ")");
  const long long need = ck_blob_bytes(mode, n, count);
  if (bytes != need)
    return ck_fail(msg, who + std::to_string(bytes) + " bytes given, " + std::to_string(count) + " records take " +
                            std::to_string(need) + " (dat_checkpoint_bytes)");
  return 0;
}

// dat_checkpoint_load's arguments against a handle of (mode, n, batch): the blob, every record index against the
// blob's count, every destination against the batch, and the destinations distinct.  [*lo, *hi): the records named.
inline int ck_check_load(int mode, int n, int batch, const void* blob, long long bytes, const int* records,
                         const int* scenarios, int count, long long* lo, long long* hi, std::string* msg) {
  const std::string who = "dat_checkpoint_load: ";
  if (count < 0) return ck_fail(msg, who + "negative count " + std::to_string(count));
  CkHeader h;
  std::string m;
  if (ck_check_header(mode, n, blob, bytes, &h, &m)) return ck_fail(msg, who + m);
  long long a = LLONG_MAX, b = 0;
  std::vector<char> seen((size_t)batch, 0);
  for (int k = 0; k < count; ++k) {
    const long long r = records ? records[k] : k;
    if (r < 0 || r >= h.count)
      return ck_fail(msg, who + "record " + std::to_string(r) + " (entry " + std::to_string(k) + ") out of range: the blob holds " +
                              std::to_string(h.count));
    const long long s = scenarios ? scenarios[k] : k;
    if (s < 0 || s >= batch)
      return ck_fail(msg, who + "scenario " + std::to_string(s) + " (entry " + std::to_string(k) + ") out of range [0, " +
                              std::to_string(batch) + ")");
    if (seen[(size_t)s]) return ck_fail(msg, who + "duplicate destination: scenario " + std::to_string(s) + " is named twice");
    seen[(size_t)s] = 1;
    a = r < a ? r : a;
    b = r + 1 > b ? r + 1 : b;
  }
  if (lo) *lo = count ? a : 0;
  if (hi) *hi = count ? b : 0;
  return 0;
}

}  // namespace dat
