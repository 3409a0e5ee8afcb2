// sl_balance_host.cpp -- the placement core of the sorted report lists (vimure_amd/csrc/sl_balance.h) as a host program:
//   c++ -O2 -std=c++17 -I vimure_amd/csrc tools/sl_balance_host.cpp -o sl_balance_host
//   (by hand, for a memory check: add -fsanitize=address,undefined)
// stdin:  records of u32 -- R, lead[64], e[R * 64] (e[r * 64 + lane]) -- until the end of the input
// stdout: per record the balanced e[R * 64] twice: two calls on two copies of the input (tests/test_sl_balance_host.py)
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "sl_balance.h"

int main() {
  unsigned R;
  SlbScratch sc;
  while (fread(&R, 4, 1, stdin) == 1) {
    if (R > (1u << 16)) { fprintf(stderr, "R = %u: not a step\n", R); return 2; }
    unsigned lead[64];
    std::vector<unsigned> e((size_t)R * 64);
    if (fread(lead, 4, 64, stdin) != 64 || fread(e.data(), 4, e.size(), stdin) != e.size()) { fprintf(stderr, "short record\n"); return 2; }
    for (int call = 0; call < 2; ++call) {
      std::vector<unsigned> w(e);
      slb_balance_step(w.data(), R, lead, &sc);
      if (fwrite(w.data(), 4, w.size(), stdout) != w.size()) return 3;
    }
  }
  return 0;
}
