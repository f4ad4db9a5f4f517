// TEST-ONLY stand-alone program around the handle's two rules (csrc/dat_modes.hpp), compiled by
// tests/test_modes_host.py with the host compiler and -fsanitize=address,undefined and run directly.
//   modes_check <manifest>
// One case per manifest line, one verdict line per case on stdout:
//   refuse <caller> <want> <open>   refusal(): want 0..3 a feature (LOG, EPISODES, TRACKING, PLANT_RP), 4 the action
//                                   CKPT_LOAD; open the set of open features, bit k = feature k.
//                                   -> "ok" or "refused: <message>"
//   plan <mode> <nsub> <bits>       loop_plan(): bit k of <bits> is the k-th boolean of LoopFacts in the order forest,
//                                   log_open, record_err, adv_on, pipe_on, fused_on, fused_sort_build, have_words,
//                                   have_tail, have_advance, have_pipe, have_lists, have_ktabs.
//                                   -> "<schedule 0..3> <tail_route> <fused> <fused_sort>"
//   wanted <mode> <nsub> <bits>     loop_plan_wanted(), same output
#include <fstream>
#include <iostream>
#include <sstream>

#include "../../distributed_aerial_transportation_amd/csrc/dat_modes.hpp"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::ifstream man(argv[1]);
  if (!man) return 2;
  static_assert(dat::FEAT_LOG == 0 && dat::FEAT_EPISODES == 1 && dat::FEAT_TRACKING == 2 && dat::FEAT_PLANT_RP == 3 &&
                    dat::ACT_CKPT_LOAD == 4,
                "the manifest's numbering");
  static_assert(dat::SCHED_SERIAL == 0 && dat::SCHED_SUB_BATCHES == 1 && dat::SCHED_OVERLAP == 2 &&
                    dat::SCHED_PIPELINE == 3,
                "the verdict's numbering");
  std::string line;
  while (std::getline(man, line)) {
    std::stringstream ls(line);
    std::string what;
    ls >> what;
    if (what == "refuse") {
      std::string caller;
      int want = 0;
      unsigned open = 0;
      ls >> caller >> want >> open;
      const std::string m = dat::refusal(caller.c_str(), want, open);
      std::cout << (m.empty() ? std::string("ok") : "refused: " + m) << "\n";
    } else if (what == "plan" || what == "wanted") {
      dat::LoopFacts f;
      unsigned bits = 0;
      ls >> f.mode >> f.nsub >> bits;
      bool* const b[] = {&f.forest,       &f.log_open,  &f.record_err, &f.adv_on,    &f.pipe_on,
                         &f.fused_on,     &f.fused_sort_build,         &f.have_words, &f.have_tail,
                         &f.have_advance, &f.have_pipe, &f.have_lists, &f.have_ktabs};
      for (unsigned k = 0; k < sizeof(b) / sizeof(b[0]); ++k) *b[k] = (bits >> k) & 1u;
      const dat::LoopPlan p = what == "plan" ? dat::loop_plan(f) : dat::loop_plan_wanted(f);
      std::cout << (int)p.schedule << " " << p.tail_route << " " << p.fused << " " << p.fused_sort << "\n";
    } else {
      return 4;
    }
  }
  return 0;
}
