// TEST-ONLY stand-alone program around the host-side checkpoint checks (csrc/dat_ckpt.hpp), compiled by
// tests/test_checkpoint_host.py with the host compiler and -fsanitize=address,undefined and run directly.
//   ckpt_check <manifest>
// One case per manifest line, one verdict line per case on stdout ("ok ..." or "error: <message>"):
//   tiles <mode> <n>                                                the table covers the record
//   header <mode> <n> <count> <out file>                            write a header (ck_put_header)
//   load <mode> <n> <batch> <blob file> <count> <records> <scenarios>  ck_check_load; lists: a,b,c or - (NULL)
//   save <mode> <n> <batch> <bytes> <count> <scenarios>             ck_check_save
// A blob is read into a heap block of exactly its size, so a read past `bytes` is an AddressSanitizer report.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>

#include "../../distributed_aerial_transportation_amd/csrc/dat_ckpt.hpp"

namespace {

bool parse_list(const std::string& s, std::vector<int>* out) {  // false: NULL
  out->clear();
  if (s == "-") return false;
  std::stringstream ss(s);
  std::string tok;
  while (std::getline(ss, tok, ',')) out->push_back(std::atoi(tok.c_str()));
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::ifstream man(argv[1]);
  if (!man) return 2;
  std::string line;
  while (std::getline(man, line)) {
    std::stringstream ls(line);
    std::string what;
    int mode = 0, n = 0;
    ls >> what >> mode >> n;
    std::string msg;
    if (what == "tiles") {
      std::cout << (dat::ck_table_tiles(mode, n) ? "ok " : "error: table does not tile the record of ")
                << dat::ck_record_words(mode, n) << "\n";
    } else if (what == "header") {
      long long count = 0;
      std::string path;
      ls >> count >> path;
      unsigned char hdr[DAT_CK_HEADER_BYTES];
      dat::ck_put_header(hdr, mode, n, count);
      std::ofstream(path, std::ios::binary).write((const char*)hdr, sizeof(hdr));
      std::cout << "ok " << dat::ck_blob_bytes(mode, n, count) << "\n";
    } else if (what == "load") {
      int batch = 0, count = 0;
      std::string path, rs, ss;
      ls >> batch >> path >> count >> rs >> ss;
      std::ifstream f(path, std::ios::binary | std::ios::ate);
      if (!f) return 3;
      const long long bytes = (long long)f.tellg();
      f.seekg(0);
      char* blob = (char*)std::malloc(bytes ? (size_t)bytes : 1);
      f.read(blob, bytes);
      std::vector<int> rec, scen;
      const bool hr = parse_list(rs, &rec), hs = parse_list(ss, &scen);
      long long lo = -1, hi = -1;
      const int rc = dat::ck_check_load(mode, n, batch, blob, bytes, hr ? rec.data() : nullptr,
                                        hs ? scen.data() : nullptr, count, &lo, &hi, &msg);
      std::free(blob);
      if (rc == 0)
        std::cout << "ok " << lo << " " << hi << "\n";
      else
        std::cout << "error: " << msg << "\n";
    } else if (what == "save") {
      int batch = 0, count = 0;
      long long bytes = 0;
      std::string ss;
      ls >> batch >> bytes >> count >> ss;
      std::vector<int> scen;
      const bool hs = parse_list(ss, &scen);
      char dummy = 0;
      const int rc = dat::ck_check_save(mode, n, batch, hs ? scen.data() : nullptr, count, &dummy, bytes, &msg);
      std::cout << (rc == 0 ? std::string("ok") : "error: " + msg) << "\n";
    } else {
      return 4;
    }
  }
  return 0;
}
