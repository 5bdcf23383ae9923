// Step-planner checker for tests/test_gkr_plan_cpu.py (test infrastructure, not
// the product): prints plan_phase's schedule (csrc/gkr_plan.hpp) for nv = 0..40.
// Arguments are name=value pairs, defaults the library's:
//   pre dround d0 d0t dtail use_tail cross dfs quads pairs host_rounds cus oct64 mall  (PlanKnobs)
//   host_ok gather                                                                   (plan_phase)
// (pre: ZK_PRELAUNCH; a phase of fewer than two rounds is never pre-enqueued, host.hpp prelaunch()).
// One line per nv:
//   nv=16 stop=16 host=4 order=0 tail=5440 tab=8192 fslog=0 steps=D0T@0:0:0:0 T33@3:3:0:0 ...
// a step as kind@first_round:np:nd:dfs; a planning error prints error=<text> instead of steps.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "gkr_plan.hpp"

using namespace zkh;

static const char* kind_name(int k) {
  switch (k) {
    case GS_ROUND0: return "ROUND0";
    case GS_SINGLE: return "SINGLE";
    case GS_DOUBLE: return "DOUBLE";
    case GS_TAIL: return "TAIL";
    case GS_DTAIL: return "DTAIL";
    case GS_D0: return "D0";
    case GS_D0T: return "D0T";
    case GS_T32: return "T32";
    case GS_T33: return "T33";
    case GS_HOST: return "HOST";
    default: return "?";
  }
}

int main(int argc, char** argv) {
  PlanKnobs k;
  bool pre = true, host_ok = false;
  uint32_t gather = 0;
  for (int a = 1; a < argc; ++a) {
    const char* eq = strchr(argv[a], '=');
    if (!eq) return 2;
    const std::string name(argv[a], eq - argv[a]);
    const unsigned long long v = strtoull(eq + 1, nullptr, 0);
    if (name == "pre") pre = v;
    else if (name == "dround") k.dround = v;
    else if (name == "d0") k.d0 = v;
    else if (name == "d0t") k.d0t = v;
    else if (name == "dtail") k.dtail = v;
    else if (name == "use_tail") k.use_tail = v;
    else if (name == "cross") k.cross_ranks = v;
    else if (name == "dfs") k.device_fs = v;
    else if (name == "quads") k.dtail_max_quads = v;
    else if (name == "pairs") k.tail_max_pairs = v;
    else if (name == "host_rounds") k.host_rounds = (uint32_t)v;
    else if (name == "cus") k.num_cus = (uint32_t)v;
    else if (name == "oct64") k.t33_oct64_min = (uint32_t)v;
    else if (name == "mall") k.mall_order = (uint32_t)v;
    else if (name == "host_ok") host_ok = v;
    else if (name == "gather") gather = (uint32_t)v;
    else return 2;
  }
  for (uint32_t nv = 0; nv <= 40; ++nv) {
    k.pre = pre && nv > 1;
    const PhasePlan pl = plan_phase(k, nv, host_ok, gather);
    printf("nv=%u stop=%u host=%u order=%u tail=%llu tab=%zu fslog=%d ", nv, pl.stop, pl.host_rounds, pl.d0t_order,
           (unsigned long long)pl.tail_elems, pl.host_tab_bytes, (int)pl.fslog);
    if (pl.error) {
      printf("error=%s\n", pl.error);
      continue;
    }
    printf("steps=");
    for (size_t s = 0; s < pl.steps.size(); ++s) {
      const GStep& st = pl.steps[s];
      printf("%s%s@%u:%d:%u:%d", s ? " " : "", kind_name(st.kind), st.i, st.np, st.nd, (int)st.dfs);
    }
    printf("\n");
  }
  return 0;
}
