// TEST-ONLY stand-alone program around the host-side episode checks (csrc/dat_episode_host.hpp), compiled by
// tests/test_episode_host.py with the host compiler and -fsanitize=address,undefined and run directly.
//   ep_check <manifest>
// One case per manifest line, one verdict line per case on stdout ("ok ..." or "error: <message>"):
//   begin <mode> <n> <blob file> <capacity> <goal_x> <bound> <max_steps> <stall_steps>   ep_check_begin ("-": null rules
//                                                                                        in place of goal_x)
//   read <first> <count> <held>                                                          ep_check_read
// A blob is read into a heap block of exactly its size, so a read past `bytes` is an AddressSanitizer report.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>

#include "../../distributed_aerial_transportation_amd/csrc/dat_episode_host.hpp"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::ifstream man(argv[1]);
  if (!man) return 2;
  std::string line;
  while (std::getline(man, line)) {
    std::stringstream ls(line);
    std::string what, msg;
    ls >> what;
    if (what == "begin") {
      int mode = 0, n = 0, capacity = 0;
      std::string path, goal;
      ls >> mode >> n >> path >> capacity >> goal;
      dat_episode_rules r = {};
      const bool have = goal != "-";
      if (have) {
        r.goal_x = std::strtod(goal.c_str(), nullptr);
        std::string bound;
        ls >> bound >> r.max_steps >> r.stall_steps;
        r.bound = std::strtod(bound.c_str(), nullptr);
        r.on_collision = r.wrap = 1;
      }
      std::ifstream f(path, std::ios::binary | std::ios::ate);
      if (!f) return 3;
      const long long bytes = (long long)f.tellg();
      f.seekg(0);
      char* blob = (char*)std::malloc(bytes ? (size_t)bytes : 1);
      f.read(blob, bytes);
      int records = -1;
      const int rc = dat::ep_check_begin(mode, n, have ? &r : nullptr, blob, bytes, capacity, &records, &msg);
      std::free(blob);
      if (rc == 0)
        std::cout << "ok " << records << "\n";
      else
        std::cout << "error: " << msg << "\n";
    } else if (what == "read") {
      int first = 0, count = 0;
      long long held = 0;
      ls >> first >> count >> held;
      const int rc = dat::ep_check_read(first, count, held, &msg);
      std::cout << (rc == 0 ? std::string("ok") : "error: " + msg) << "\n";
    } else {
      return 4;
    }
  }
  return 0;
}
