// sl_balance.h -- which of a tie's reports sits in which round of its step (sorted report lists, sweep_sl.h), chosen so that the 64
// lanes of a round spread over the LDS banks.  Plain C++ for a host program, __host__ __device__ under hipcc: k_sl_balance
// (sorted_lists.hip) and tests/test_sl_balance_host.py run the same code.
//
// Per report the K = 2 sweep issues two LDS instructions whose address is the report's table row ym = y * Mp + m: a 16-byte read
// of F[ym] and an 8-byte add into Hc[k * hcm + ym].  The cost model (the bank rules of the LDS):
//   read: served in four groups of 16 lanes -- {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the two shifted by 32; the bank slot
//         of a 16-byte row is ym mod 16; lanes on one row share a cycle, every further row on a slot costs one;
//   add:  four contiguous groups of 16 lanes, slot ym mod 16 again (hcm is a multiple of 64), every lane on a slot costs a cycle.
// A round costs, per instruction, the sum over its groups of the fullest slot; 4 is the least.  Empty entries issue nothing that
// the model counts.
//
// The placement permutes every lane's column and nothing else.  A column is [lead far entries | near entries | empty entries]
// (lead: the entries k_far_first moved to the front); each of the two segments is permuted within itself, and within windows of
// SLB_WIN consecutive rounds only -- the register ring of a long step walks 8 rounds at a time, and the cost stays linear in R.
// It is a pure function of its input: lanes in a fixed order, no atomics that could reach the result -- two handles of the same
// data hold the same lists.
//
// Order of the lanes.  A lane touches the counts of its read group and of its contiguous group only, so the 64 lanes fall into 8
// sets of 8 -- per half {0-3, 12-15}, {4-11}, {16-19, 28-31}, {20-27} -- of which the first and third (and the second and fourth)
// share no count, nor does anything across the halves: SLB_CHAINS chains of 8 lanes can run side by side in each of two phases
// and give what one thread gives that takes the chains one after the other.  The kernel does the former, a host the latter.
#ifndef VMR_SL_BALANCE_H
#define VMR_SL_BALANCE_H

#if defined(__HIPCC__)
#define SLB_HD __host__ __device__
#else
#define SLB_HD
#endif

#define SLB_WIN 8
#define SLB_CHAINS 4
#define SLB_ROW(e) ((e) & 0xfffffu)   // (SL_YM of sweep_sl.h)

// working memory of one window: lanes per (round, group, slot) -- the read's groups, then the contiguous ones
struct SlbScratch {
  unsigned char cr[SLB_WIN][4][16];
  unsigned char ca[SLB_WIN][4][16];
  unsigned in[SLB_WIN * 64];   // the window as it came
};

SLB_HD inline int slb_read_group(int lane) {
  const int q = lane & 31;
  return ((lane >> 5) << 1) | (int)((0xf00f0ff0u >> q) & 1u);   // lanes 4-11, 16-19, 28-31 of a half: its second group
}

// the i-th lane (i < 16, ascending) of read group g
SLB_HD inline int slb_group_lane(int g, int i) {
  const int q = (g & 1) ? (i < 8 ? i + 4 : (i < 12 ? i + 8 : i + 16)) : (i < 4 ? i : (i < 8 ? i + 8 : i + 12));
  return ((g >> 1) << 5) + q;
}

// the i-th lane (i < 8) of chain c (< SLB_CHAINS) in phase p (< 2)
SLB_HD inline int slb_chain_lane(int p, int c, int i) {
  const int half = (c >> 1) << 5, upper = (c & 1) << 4;   // chains 0, 1: lanes 0-31, chains 2, 3: 32-63; odd chains: the upper 16 of the half
  const int q = p == 0 ? (i < 4 ? i : i + 8) : i + 4;     // {0-3, 12-15} | {4-11} of a group of 16
  return half + upper + q;
}

// whether lane's entry of the round w[64] puts a new row on its read group: no lower lane of the group holds the same row
// (all 16 lanes of the group are looked at, without an early way out: 16 independent loads)
SLB_HD inline bool slb_opens_row(const unsigned* w, int lane) {
  const unsigned e = w[lane];
  const int g = slb_read_group(lane);
  bool dup = false;
  for (int i = 0; i < 16; ++i) {
    const int j = slb_group_lane(g, i);
    const unsigned o = w[j];
    dup = dup || (j < lane && o != 0u && SLB_ROW(o) == SLB_ROW(e));
  }
  return e != 0u && !dup;
}

// cycles of one round under the model: rd / ad += sum over the groups of the fullest slot.  w: the round's 64 entries.
// (a host's way; the kernel counts the same with one thread per lane)
inline void slb_round_cost(const unsigned* w, unsigned* rd, unsigned* ad) {
  unsigned nrow[4][16] = {}, nlane[4][16] = {};
  for (int lane = 0; lane < 64; ++lane) {
    if (w[lane] == 0u) continue;
    const unsigned s = SLB_ROW(w[lane]) & 15u;
    ++nlane[lane >> 4][s];
    if (slb_opens_row(w, lane)) ++nrow[slb_read_group(lane)][s];
  }
  for (int g = 0; g < 4; ++g) {
    unsigned mr = 0u, ma = 0u;
    for (int s = 0; s < 16; ++s) { mr = nrow[g][s] > mr ? nrow[g][s] : mr; ma = nlane[g][s] > ma ? nlane[g][s] : ma; }
    *rd += mr; *ad += ma;
  }
}

// One lane of a window, greedy: every entry of sc->in's column to the free round of its segment whose slot holds the fewest lanes
// so far (both groupings; the lowest such round).  w[r * 64 + lane], r < nr <= SLB_WIN; segments [0, lead) and [lead, n).
SLB_HD inline void slb_place_lane(unsigned* w, int nr, int lane, unsigned lead, unsigned n, SlbScratch* sc) {
  const int gr = slb_read_group(lane), ga = lane >> 4;
  const int nl = (int)n < nr ? (int)n : nr, ld = (int)lead < nl ? (int)lead : nl;
  for (int seg = 0; seg < 2; ++seg) {
    const int lo = seg ? ld : 0, hi = seg ? nl : ld;
    unsigned used = 0u;
    for (int i = lo; i < hi; ++i) {
      const unsigned e = sc->in[i * 64 + lane], s = SLB_ROW(e) & 15u;
      int best = -1; unsigned bc = 0u;
      for (int r = lo; r < hi; ++r) {
        const unsigned c = (unsigned)sc->cr[r][gr][s] + (unsigned)sc->ca[r][ga][s];
        if (!((used >> r) & 1u) && (best < 0 || c < bc)) { best = r; bc = c; }
      }
      used |= 1u << best;
      w[best * 64 + lane] = e;
      ++sc->cr[best][gr][s]; ++sc->ca[best][ga][s];
    }
  }
}

// ... and the refinement: the lane swaps two of its entries where that lowers the sum of the squared slot counts
SLB_HD inline void slb_refine_lane(unsigned* w, int nr, int lane, unsigned lead, unsigned n, SlbScratch* sc) {
  const int gr = slb_read_group(lane), ga = lane >> 4;
  const int nl = (int)n < nr ? (int)n : nr, ld = (int)lead < nl ? (int)lead : nl;
  for (int seg = 0; seg < 2; ++seg) {
    const int lo = seg ? ld : 0, hi = seg ? nl : ld;
    for (int a = lo; a < hi; ++a)
      for (int b = a + 1; b < hi; ++b) {
        const unsigned ea = w[a * 64 + lane], eb = w[b * 64 + lane], sa = SLB_ROW(ea) & 15u, sb = SLB_ROW(eb) & 15u;
        if (sa == sb) continue;
        // the other lanes on the four slots: the swap moves sa to round b and sb to round a
        const int now = (int)sc->cr[a][gr][sa] + (int)sc->ca[a][ga][sa] + (int)sc->cr[b][gr][sb] + (int)sc->ca[b][ga][sb] - 4;
        const int then = (int)sc->cr[a][gr][sb] + (int)sc->ca[a][ga][sb] + (int)sc->cr[b][gr][sa] + (int)sc->ca[b][ga][sa];
        if (then < now) {
          --sc->cr[a][gr][sa]; --sc->ca[a][ga][sa]; --sc->cr[b][gr][sb]; --sc->ca[b][ga][sb];
          ++sc->cr[a][gr][sb]; ++sc->ca[a][ga][sb]; ++sc->cr[b][gr][sa]; ++sc->ca[b][ga][sa];
          w[a * 64 + lane] = eb; w[b * 64 + lane] = ea;
        }
      }
  }
}

// Chain c of a window: the greedy pass (refine = false) or the refinement over its lanes, phase after phase.  Needs sc->in = the
// window as it came, w = the same, the counts zero before the greedy pass; every chain's greedy pass before any refinement.
// Chains may run side by side; between the phases every chain must have finished the one before (a barrier).
SLB_HD inline void slb_chain_phase(unsigned* w, int nr, const unsigned* lead, const unsigned* n, SlbScratch* sc, int c, int p, bool refine) {
  for (int i = 0; i < 8; ++i) {
    const int lane = slb_chain_lane(p, c, i);
    if (refine) slb_refine_lane(w, nr, lane, lead[lane], n[lane], sc);
    else slb_place_lane(w, nr, lane, lead[lane], n[lane], sc);
  }
}

// One window on one thread: w[r * 64 + lane], r < nr <= SLB_WIN.  Lane's entries of rounds [0, lead[lane]) stay there, those of
// [lead[lane], n[lane]) too; rounds from n[lane] on are empty and stay empty.  The result is never worse than the input under the
// model, for the read and for the add (else the window is left as it came).
inline void slb_balance_window(unsigned* w, int nr, const unsigned* lead, const unsigned* n, SlbScratch* sc) {
  if (nr < 2) return;
  for (int i = 0; i < nr * 64; ++i) sc->in[i] = w[i];
  for (int r = 0; r < nr; ++r)
    for (int g = 0; g < 4; ++g)
      for (int s = 0; s < 16; ++s) { sc->cr[r][g][s] = 0; sc->ca[r][g][s] = 0; }
  for (int pass = 0; pass < 2; ++pass)
    for (int p = 0; p < 2; ++p)
      for (int c = 0; c < SLB_CHAINS; ++c) slb_chain_phase(w, nr, lead, n, sc, c, p, pass == 1);
  unsigned r0 = 0u, a0 = 0u, r1 = 0u, a1 = 0u;
  for (int r = 0; r < nr; ++r) { slb_round_cost(sc->in + r * 64, &r0, &a0); slb_round_cost(w + r * 64, &r1, &a1); }
  if (r1 > r0 || a1 > a0)
    for (int i = 0; i < nr * 64; ++i) w[i] = sc->in[i];
}

// what a window starting at round r0 sees of a lane's segment bounds
SLB_HD inline unsigned slb_clip(unsigned v, unsigned r0) { return v > r0 ? v - r0 : 0u; }

// A lane's report count: one past its last entry that is not empty.  col: the lane's column, stride 64.
SLB_HD inline unsigned slb_count(const unsigned* col, unsigned R) {
  unsigned n = 0u;
  for (unsigned r = 0; r < R; ++r) if (col[(unsigned long long)r * 64] != 0u) n = r + 1;
  return n;
}

// One whole step in place: e[r * 64 + lane], r < R; lead[lane] as above (at most the lane's report count).
inline void slb_balance_step(unsigned* e, unsigned R, const unsigned* lead, SlbScratch* sc) {
  unsigned n[64], lw[64], nw[64];
  for (int lane = 0; lane < 64; ++lane) n[lane] = slb_count(e + lane, R);
  for (unsigned r0 = 0; r0 < R; r0 += SLB_WIN) {
    const unsigned nr = R - r0 < SLB_WIN ? R - r0 : SLB_WIN;
    for (int lane = 0; lane < 64; ++lane) { lw[lane] = slb_clip(lead[lane] < n[lane] ? lead[lane] : n[lane], r0); nw[lane] = slb_clip(n[lane], r0); }
    slb_balance_window(e + (unsigned long long)r0 * 64, (int)nr, lw, nw, sc);
  }
}

#endif
