// Launch plan of the row-banded weight-gradient kernel (usf_conv_wgrad_band.hip): ONE statement of the band, the LDS geometry,
// the instantiation, the grid and the reduction.  The entry point launches from it and usf_conv_wgrad_band_variant answers from
// it.  Host code without a HIP call: a pure function of the sizes, the compute-unit count and the two caps.
#ifndef USF_CONV_WGRAD_BAND_PLAN_H
#define USF_CONV_WGRAD_BAND_PLAN_H
#include <stdint.h>

namespace usf {

constexpr int kWbLdsMax = 160 * 1024;
constexpr int kWbReduceRows = 64;       // scratch rows of the two-round sum (workspace: that many * nacc floats behind the slots)
constexpr int kWbOnesLead = 64;         // the bias operand's row is this much longer than CSx: column j of the tile reads it 4 * j floats earlier
constexpr int kWbMinRows = 4;           // the plan never lowers a band below this many rows on its own (the halo would pass half the band)

struct WbPlan {
  int CIT, COT, T, pad, S, q0, xbase;   // tiles, taps, halo rows, row stride, position of pixel (r0, 0) / of the first staged pixel in x
  int RB, RB_best, RB_fit;              // band rows of this launch, the plan's own choice, the most the LDS holds
  int nbands, last_rows, XR;            // bands per sample, rows of a sample's last band, staged x rows of a full band (RB + 2 pad)
  int nch, CSx, CSy, lds_floats, lds_bytes;
  int ntiles, TG, PS, NT, nacc;
  int groups, blocks, slots, per_cu, cus;
  unsigned m_x, m_y, m_w;               // ceil(2^32 / d) for d = XR * W, RB * W, W (0: d == 1)
  int max_e;                            // the largest dividend the kernel divides with m_x / m_y (m_w: below XR * W)
};

// n / d = umulhi(n, wb_magic(d)) for every n with n * d < 2^32 (the plan's dividends stay below 2^19, its divisors below 2^13)
inline unsigned wb_magic(int d) { return d < 2 ? 0u : (unsigned)((0x100000000ULL + (unsigned)d - 1) / (unsigned)d); }

inline int wb_two_odd_at_least(int need) {
  int h = (need + 1) / 2;
  if (!(h & 1)) ++h;
  return 2 * h;
}

// the LDS geometry of a band of RB rows: kernel 3 keeps the wide kernel's layout (row stride W + 1, a zero row above and below
// the RB + 2 staged x rows), kernel 1 the plain one
inline void wb_geometry(int W, int ks, int RB, WbPlan& pl) {
  if (ks == 3) {
    pl.pad = 1;
    pl.S = W + 1;
    pl.q0 = pl.S + 1;
    pl.nch = ((RB - 1) * pl.S + W + 3) / 4;                         // padded positions from the band's first to its last pixel, in fours
    pl.CSy = wb_two_odd_at_least(4 * pl.nch);
    pl.CSx = wb_two_odd_at_least(pl.q0 + 4 * pl.nch + pl.S + 1);    // last position a fragment read touches + 1
  } else {
    pl.pad = 0;
    pl.S = W;
    pl.q0 = 0;
    pl.nch = (RB * W + 3) / 4;
    pl.CSx = pl.CSy = wb_two_odd_at_least(4 * pl.nch);
  }
  pl.xbase = pl.q0 - pl.pad * pl.S;
  // (+ the bias tile's B operand: a row of CSx + kWbOnesLead floats, ones in every 16th position chunk)
  pl.lds_floats = (pl.CIT * 16 + 1) * pl.CSx + kWbOnesLead + pl.COT * 16 * pl.CSy;
  pl.lds_bytes = pl.lds_floats * 4;
}

// rounds of the sum of `nparts` slots: 1 up to 64 slots; else 2: a first round of `used` rows (<= 64) of `per` slots each
inline int wb_rounds(int nparts, int& per, int& used) {
  per = nparts;
  used = 1;
  if (nparts <= 64) return 1;
  const int rows = nparts / 16 < kWbReduceRows ? (nparts + 15) / 16 : kWbReduceRows;
  per = (nparts + rows - 1) / rows;
  used = (nparts + per - 1) / per;
  return 2;
}

// The band: RB_fit = the most rows whose image fits the 160 KiB; not served when kernel 3 gets fewer than kWbMinRows rows of a
// map that has more (W = 64 at 49 + 64 channels and up: the halo rows would outweigh the band).  A batch whose groups would
// leave compute units idle takes a lower band, down to kWbMinRows rows, and the bands are evened out (28 rows in bands of
// 19 + 9 become 14 + 14); band_rows > 0 caps the result as it is.  The grid: min(groups, cus * min(blocks_per_cu, 2)), under
// block_cap when that is > 0.  cus > 0; blocks_per_cu <= 0: what the LDS image allows.  Neither the lower band nor the second
// block per compute unit is measured against its alternative; the second block counts LDS alone: the instantiations of 19 tiles
// per wave and more hold one or two waves per SIMD in registers, so there a second block may only queue (its slot costs a
// little of the sum, nothing else).
inline bool wgrad_band_plan(int64_t B, int64_t cin, int64_t cout, int64_t H_, int64_t W_, int64_t ks, int band_rows, int cus,
                            int blocks_per_cu, int block_cap, WbPlan& pl) {
  pl = WbPlan();
  if (B <= 0 || B > 0x7fffffff || cin <= 0 || cout <= 0 || cin > 64 || cout > 64 || H_ <= 0 || W_ <= 0 || W_ > 64 || H_ > 4096 ||
      H_ * W_ > 4096 || (ks != 1 && ks != 3) || band_rows < 0 || cus <= 0)
    return false;
  const int H = (int)H_, W = (int)W_;
  pl.CIT = (int)(cin + 15) / 16;
  pl.COT = (int)(cout + 15) / 16;
  pl.T = (int)(ks * ks);
  int fit = 0;
  for (int rb = H; rb >= 1; --rb) {
    wb_geometry(W, (int)ks, rb, pl);
    if (pl.lds_bytes <= kWbLdsMax) { fit = rb; break; }
  }
  pl.RB_fit = fit;
  if (fit < 1 || (ks == 3 && fit < kWbMinRows && fit < H)) return false;
  int RB = fit;
  if (B * ((H + RB - 1) / RB) < cus && RB > kWbMinRows) {          // idle compute units: more, lower bands
    const int64_t want = (cus + B - 1) / B;                          // bands per sample that give every compute unit a group
    const int rb = (int)((H + want - 1) / want);
    RB = rb < kWbMinRows ? kWbMinRows : (rb < RB ? rb : RB);
  }
  RB = (H + (H + RB - 1) / RB - 1) / ((H + RB - 1) / RB);             // the same number of bands, evened out
  pl.RB_best = RB;
  if (band_rows > 0 && band_rows < RB) RB = band_rows;
  pl.RB = RB;
  pl.nbands = (H + RB - 1) / RB;
  pl.last_rows = H - (pl.nbands - 1) * RB;
  wb_geometry(W, (int)ks, RB, pl);
  pl.XR = RB + 2 * pl.pad;
  if (B * pl.nbands > 0x7fffffff) return false;
  pl.groups = (int)(B * pl.nbands);
  pl.ntiles = pl.COT * (pl.CIT * pl.T + 1);                          // (+ one bias tile per cout tile)
  pl.TG = pl.ntiles >= 3 ? 4 : pl.ntiles;
  pl.PS = 4 / pl.TG;
  pl.NT = (pl.ntiles + pl.TG - 1) / pl.TG;
  pl.nacc = pl.ntiles * 256;
  int per_cu = blocks_per_cu > 0 ? blocks_per_cu : kWbLdsMax / pl.lds_bytes;
  pl.per_cu = per_cu;
  if (per_cu > 2) per_cu = 2;                                         // (more partial slots than that buy nothing)
  pl.cus = cus;
  int64_t blocks = pl.groups;
  if (blocks > (int64_t)cus * per_cu) blocks = (int64_t)cus * per_cu;
  if (block_cap > 0 && blocks > block_cap) blocks = block_cap;
  pl.blocks = (int)blocks;
  pl.slots = pl.blocks * pl.PS;
  pl.m_x = wb_magic(pl.XR * W);
  pl.m_y = wb_magic(RB * W);
  pl.m_w = wb_magic(W);
  const int cmax = (int)(cin > cout ? cin : cout);
  pl.max_e = cmax * pl.XR * W - 1;
  return true;
}

}  // namespace usf
#endif
