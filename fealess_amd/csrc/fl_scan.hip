// fl_scan.hip -- the coarse scan of the online matching half of cup_linemod::Detector over the linear memories
// fl_linmem.hip lays out (reference: linemod/linemod.cpp:882-1577).
//
//   k_scan         similarity + addSimilarities + coarse threshold          (:1130-1214, 1322-1338, 1483-1506)
#include "fl_internal.h"

// ------------------------------------------------------------------------------------------
// k_scan: one wavefront per run of (pyramid, 1024-position chunk) work items of a frame.  Lane i owns 16 consecutive
// positions and keeps their u8 partial sums packed in four 32-bit registers per modality:
// with <= 63 features of response <= 4 a byte never carries (63*4 = 252, linemod.cpp:1133-1137),
// so one 32-bit add sums four positions.  Feature offsets are wave-uniform (scalar loads), padded
// to a multiple of 8 with the offset of the zero pad so that 8 independent 16-byte loads are in
// flight per step.  The linear memories (1.2 MB per frame at VGA/T=8) are shared by all
// templates and are served from L2; the feature tables are the only per-template HBM stream.
// Between the modalities and after every 8 features a wave whose positions can no longer reach the coarse threshold stops
// (exact: see `prune` in the kernel); the reference adds every feature of every template everywhere (linemod.cpp:1471-1481).
//
// With pruning most items end after 16 of up to 126 features, and what such an item costs is not its bytes but the chain
// of dependent memory round trips in front of them.  So everything an item needs before its first vector load is one
// 64-byte record (FlScanItem, built at finalize: it depends on the bank and the geometry only) with the first eight
// offsets inline; the class filter's flag is a byte per ITEM, requested with the record; a wave walks `run` items
// (ScanArgs::run, fl_scan_run) and requests the next item's record and flag before it works on the current one; and
// inside an item the next group's eight offsets -- the next modality's first group behind a modality's last -- are
// requested before the current group's vector loads are waited for.  An early-pruned item then costs the two vector
// round trips of its two groups; the record, the flag and the offsets arrive underneath them.
//
// The bound is per lane (a lane's own 16 positions), so a lane that misses it stops loading for itself (ScanArgs::prune_lanes),
// and behind a modality's first eight features the checks come every STEP features (the kernel's second template parameter,
// fl_scan_step): see `alive` in the kernel.  What this buys is load instructions and lanes not issued; the launch is NOT bound by
// the vector cache's line lookups (a quarter fewer of them moved the time by 1 %, profiles/README.md).  What did bind it was the
// scalar cache: lane 63's tail dword, one scalar load per feature at an address all over the linear memories, is now fetched
// only where lane 63 loads.
struct ScanArgs {
  const FlScanItem *items;   // work list: one record per (pyramid, chunk)
  int n_items;
  const uint32_t *offs;      // FL_SCAN_OFF_PAD entries behind the last group
  const uint8_t *enabled;    // per work item, whole dwords: class selected by match()'s class_ids (linemod.cpp:1418-1434)
  uint8_t *ws;               // frame workspace base
  size_t ws_stride;
  size_t lm_off[FL_MAX_MODALITIES];
  size_t off_count, off_cand;
  int M, W, WH, T, cap;
  int bpf, n_frames;         // blocks per frame, frames in this launch
  int run, wave_step, item_step;   // wave w of a frame walks the items w * wave_step + i * item_step, i < run
  float threshold;
  int prune;                 // stop a (template, chunk) between modalities once no position can reach the threshold (exact)
  unsigned prune_mid;        // ... and inside a modality after the 8-feature groups whose bit is set (same bound, same exactness)
  int prune_lanes;           // a lane whose own 16 positions miss the bound stops loading (0: the wave stops as a whole or not at all)
  uint16_t *dbg;             // optional raw u16 maps of pyramids [dbg_first, dbg_first+dbg_count); null: dbg_count = 0
  int dbg_first, dbg_count;
};

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
// the larger even byte and the larger odd byte of a word, as two 16-bit values (v_pk_max_u16)
__device__ __forceinline__ u16x2 pk_bytes_max(uint32_t a)
{
  const uint32_t lo = a & 0x00FF00FFu, hi = (a >> 8) & 0x00FF00FFu;
  return __builtin_elementwise_max(__builtin_bit_cast(u16x2, lo), __builtin_bit_cast(u16x2, hi));
}
// a wave-uniform load of memory no kernel in flight writes: s_load_dword whatever stores the loop holds
#define FL_CONST_AS __attribute__((address_space(4)))
__device__ __forceinline__ uint32_t sload1(const void *p) { return *(const FL_CONST_AS uint32_t *)(uintptr_t)p; }
// What the loop keeps in flight for later -- the next item's record and flag, the next group's offsets -- travels in ONE vector
// register each, a dword per lane, and is taken apart with v_readlane when its turn comes: sixteen and eight scalar registers
// held across an item were more than the scalar file has beside the group in work (the compiler then issued a group's loads
// one at a time).  Vector loads return in order, so the wait for a group's own loads covers the request issued before them.
__device__ __forceinline__ uint32_t rl(uint32_t v, int l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, l); }

#ifndef FL_SCAN_PRUNE_MID
#define FL_SCAN_PRUNE_MID 0x7Fu   // 8-feature groups after which a modality checks the bound (every one but the last: the check
                                  // after 16 features is the one that pays -- chunks without colour edges stop there)
#endif
// Waves per SIMD.  Without pruning the kernel is bound by the rate of its vector loads and five waves are the optimum (measured
// after the DPP change, ms per 1280 frames x 360 templates: 3: 2.32, 4: 1.95, 5: 1.71, 6: 1.77, 8: 2.17).  With pruning an item is
// two or three round trips and little else, the launch is bound by how many of them are in flight, and six beat five, eight
// beat seven where the first piece is short (profiles/README.md): the same code built twice, the launch picks by ScanArgs::prune.
#ifndef FL_SCAN_WPE
#define FL_SCAN_WPE 5
#endif
#ifndef FL_SCAN_WPE_PRUNED
#define FL_SCAN_WPE_PRUNED 8
#endif
// (The attribute makes the compiler pad a build's register allocation to its waves: a build for fewer than eight waves holds
// fewer although its code fits 64 vector and 80 scalar registers.)
#ifndef FL_SCAN_STEP
#define FL_SCAN_STEP 4            // feature loads between two checks behind a modality's first eight (option scan_prune_step: 8, 4 or 2)
#endif
#ifdef FL_SCAN_STATS
// development aid: per launch {items, feature-load instructions, lane-loads (lanes in EXEC), items that ran to their end}, then
// the items ended by a check after f features of all modalities (f = 0 .. 126); printed by the launcher after a stream
// synchronisation (tools/dev/README.md)
#define FL_SCAN_STATS_N (4 + 2 * FL_MAX_FEATURES + 1 + 1)
__device__ unsigned long long d_scan_stats[FL_SCAN_STATS_N];
#define FL_SCAN_STAT(i, v) do { if (lane == 0) atomicAdd(&d_scan_stats[i], (unsigned long long)(v)); } while (0)
#else
#define FL_SCAN_STAT(i, v) do { } while (0)
#endif
template <int N> struct ScanInt { static constexpr int value = N; };
// STEP: behind a modality's first piece, the feature loads between two checks of the bound (8, 4 or 2)
// FIRST: the features of a modality's first piece, which has one check, behind it (8, 12, 14 or 16; fl_scan_first)
template <int WPE, int STEP, int FIRST>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(WPE, WPE))) void k_scan(ScanArgs a)
{
  static_assert(STEP == 8 || STEP == 4 || STEP == 2, "a group of eight offsets is cut into equal parts");
  static_assert(FIRST == 8 || FIRST == 12 || FIRST == 14 || FIRST == 16, "the first piece ends inside the second group, at an even feature");
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  // XCD-aware block mapping: workgroups are dealt round-robin over the 8 XCDs, each with its own
  // 4 MB L2.  All blocks of one frame are given the same residue mod 8, so a frame's linear
  // memories (1.2 MB at VGA level 1) are fetched into ONE L2 and reused by every template there,
  // instead of being streamed into all eight.  Placement only affects speed, never results.
  const int xcd = blockIdx.x & 7, q = blockIdx.x >> 3;
  const int frame = xcd + 8 * (q / a.bpf);
  if (frame >= a.n_frames) return;
  int it = __builtin_amdgcn_readfirstlane(((q % a.bpf) * 4 + wave) * a.wave_step);
  if (it >= a.n_items) return;
  // lanes 0..15: the dwords of item `idx`'s record; the others: the dword that holds its class-filter flag
  const int l7 = lane & 7;
  // What only an item with candidates or a tapped one needs is read from the kernel arguments when it is needed: in scalar
  // registers for the whole loop it would crowd out the offsets and records the loop keeps in flight, and above 80 scalar
  // registers a SIMD holds seven waves, not eight.  (Not what EVERY item needs: a scalar load in front of an item's first
  // vector loads is a round trip of its own -- the switches read per item made the launch 14 % slower.)
  const FL_CONST_AS ScanArgs *ka = (const FL_CONST_AS ScanArgs *)__builtin_amdgcn_kernarg_segment_ptr();
  auto kargs = [&]() {
    const FL_CONST_AS ScanArgs *kr = ka;
    asm volatile("" : "+s"(kr));
    return kr;
  };
  auto request_item = [&](int idx) {
    const uint32_t *p = lane < 16 ? (const uint32_t *)(a.items + idx) + lane : (const uint32_t *)(a.enabled + (idx & ~3));
    return *p;
  };
  // the launch's switches in one scalar register: bits 0..7 the mask of the groups with checks, then F_*
  enum : unsigned { F_PRUNE = 0x100u, F_BY_LANE = 0x200u, F_TAPPED = 0x400u, F_TAPS = 0x800u, F_M2 = 0x1000u };
  const unsigned kflags = (a.prune ? F_PRUNE | (a.prune_mid & 0xFFu) | (a.prune_lanes ? F_BY_LANE : 0u) : 0u) | (a.dbg_count ? F_TAPS : 0u) |
                          (a.M > 1 ? F_M2 : 0u);
  uint32_t rec = request_item(it);
  const uint8_t *lm[FL_MAX_MODALITIES];                  // the frame's linear memories
  for (int m = 0; m < FL_MAX_MODALITIES; ++m) lm[m] = a.ws + (size_t)frame * a.ws_stride + a.lm_off[m];
  const float thr100 = a.threshold / 100.f;
  const unsigned lane_off = (unsigned)lane * 16u;

  // One work item.  `return` = on to the wave's next item; every per-item value starts from zero in here.
  auto scan_item = [&](const uint32_t r) {
    // The record stays in its vector register for the whole item and a field is read from it (v_readlane) where it is used:
    // all of them in scalar registers from the start were nine held for modality 1 and the emission while modality 0 runs.
    auto field = [&](int i) {
      uint32_t rr = r;
      asm volatile("" : "+v"(rr));
      return rl(rr, i);
    };
    const int g = (int)rl(r, 8), chunk = (int)(rl(r, 9) & 0xFFFFu), nf_all = (int)(rl(r, 9) >> 16);
    const int j0 = chunk * 1024 + lane * 16;

    // The lane's 16 totals, two per register: a total is at most 4 x 126 = 504, so position 4 q + b sits in the 16-bit half
    // b >> 1 of tp[2 q + (b & 1)] -- the even and the odd bytes of accumulator word q, each added with one 32-bit add that never
    // carries from one half into the other.  Eight registers instead of sixteen are what lets the kernel live in 64.
    uint32_t tp[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) tp[i] = 0;
    auto tot_at = [&](int i) { return (tp[2 * (i >> 2) + (i & 1)] >> (((i >> 1) & 1) * 16)) & 0xFFFFu; };
    auto tot_max = [&]() {                                 // the lane's largest total (v_pk_max_u16)
      u16x2 m = __builtin_bit_cast(u16x2, tp[0]);
#pragma unroll
      for (int i = 1; i < 8; ++i) m = __builtin_elementwise_max(m, __builtin_bit_cast(u16x2, tp[i]));
      return (uint32_t)max(m.x, m.y);
    };
    // Exact pruning between modalities: a feature adds at most 4 to a position (SIMILARITY_LUT's largest entry), so once the
    // largest total of this wave's 1024 positions plus 4 x (the features of the modalities still to come) cannot exceed the
    // coarse threshold, no position of the chunk can become a candidate (`raw > raw_threshold`, linemod.cpp:1490-1492) and the
    // rest of the template's additions have no observable effect: the item ends.  The colour modality comes first and is
    // sparse (gradients only on edges), so on most (template, chunk) pairs the depth modality -- half of the scan's loads -- is
    // never read.  The same bound is checked inside a modality after the 8-feature groups a.prune_mid names (chunks without
    // colour edges stop after 16 features).  Not when the raw maps are tapped (fl_similarity_maps), and FL_SCAN_PRUNE=0
    // switches it off (a.prune).
    const int prune_threshold = (int)(2 * nf_all + thr100 * (2 * nf_all) + 0.5f);   // = raw_threshold below
    // The item's switches live in ONE scalar register and are tested where they are used: as booleans of their own the
    // compiler keeps each in a register pair from here to the item's end.  A tapped item (only a launch with taps can have
    // one) does not prune.
    unsigned flags_ = kflags;
    const unsigned flags_m2 = kflags & F_M2;
    if (kflags & F_TAPS) {
      const FL_CONST_AS ScanArgs *ki = kargs();
      if ((unsigned)(g - ki->dbg_first) < (unsigned)ki->dbg_count) flags_ = F_TAPPED | flags_m2;
    }
    const unsigned flags = flags_;
    auto flag = [&](unsigned bits) {
      unsigned f = flags;
      asm volatile("" : "+s"(f));
      return (f & bits) != 0u;
    };
    // Per lane: the bound is computed for a lane's own 16 positions, so a lane that misses it can stop for itself.  `alive`
    // holds the lanes that still own a reachable position, wave-uniform in a scalar register pair.  A check removes lanes and
    // never brings one back; the item ends when none is left.  The loads of the groups that follow run under
    // alive | alive << 1 (a lane's bytes 16..19 are its upper neighbour's first dword), so a dead lane's accumulators go
    // stale or, next to a live lane, take in a wrong tail: it has no say in later checks and is kept out of the emission.
    // (Even unguarded it could not emit where its tail is right: its stale totals are below its true totals, which are below
    // the threshold.)  Without a.prune_lanes a check keeps every lane or none, the wave-wide rule.
    uint64_t alive = ~0ull;
    auto still = [&](bool reachable) {                     // one check: false = the item is over
      const uint64_t b = __ballot(reachable) & alive;
      alive = flag(F_BY_LANE) || b == 0ull ? b : ~0ull;
      return alive != 0ull;
    };
    [[maybe_unused]] int f_done = 0;                                     // (FL_SCAN_STATS: features added so far)
    FL_SCAN_STAT(0, 1);
    // the group of eight offsets in flight (lanes 0..7) and where in a.offs it is from: the record brings modality 0's first
    uint32_t ov = r;
    int o_at = (rl(r, 12) & 0xFFFFu) ? (int)rl(r, 11) : -1;
    int nf = 0;
#pragma unroll
    for (int m = 0; m < FL_MAX_MODALITIES; ++m) {
      if (m > 0 && !flag(F_M2)) break;                     // (FL_MAX_MODALITIES is 2)
      const uint32_t rN = m == 0 ? rl(r, 12) : field(12 + 3 * m);
      const int P = (int)(m == 0 ? rl(r, 10) : field(10 + 3 * m)), off_begin = (int)(m == 0 ? rl(r, 11) : field(11 + 3 * m));
      const int n_pad = (int)(rN & 0xFFFFu), h_nf = (int)(rN >> 16);
      uint32_t mx_tot = 0;                                 // the lane's largest total of the modalities done
      if (m > 0 && flag(F_PRUNE)) {
        mx_tot = tot_max();
        if (!still((int)mx_tot + 4 * (nf_all - nf) > prune_threshold)) {                      // wave-uniform
          FL_SCAN_STAT(4 + f_done, 1);
          return;
        }
      }
      nf += h_nf;
      if (chunk * 1024 >= P) continue;                    // wave-uniform; lanes past P load along (masked below): the
                                                         // next lane's first dword is this lane's bytes 16..19
      const uint8_t *lm_u = lm[m] + chunk * 1024;         // lane 0's bytes: wave-uniform
      // descriptor over the frame's linear memories from 4 bytes below this chunk on (scalar offsets stay positive)
      const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)(lm_u - 4), 0, 0x7FFFFFFF, 0x00020000);
      uint32_t a0 = 0, a1 = 0, a2 = 0, a3 = 0;
      // A feature's 16 bytes start at an arbitrary byte.  A byte-aligned 16-byte load costs ~2.4x a 4-byte aligned one
      // on gfx950 (tools/probes/ldwidth.hip) and this loop is bound by exactly those loads, so each feature is fetched as
      // an aligned 16 + 4 bytes and shifted into place with four v_alignbyte (the misalignment is wave-uniform).
      // The extra 4 bytes are the next lane's first dword: one DPP wave shift instead of a second vector load; lane 63's
      // come from a wave-uniform address, i.e. a scalar load.
      const unsigned lm_mis = (unsigned)(size_t)lm_u & 3u;  // same for every lane (lane * 16): keep it a scalar
      // Only the lanes whose 16 positions start below template_positions have anything to add (P = 831 of the 1024 positions
      // of a chunk for a 160-pixel template at VGA level 1: 52 of 64 lanes); one more lane stays on because its first dword is
      // the previous lane's bytes 16..19.  The condition is a contiguous lane range, i.e. one EXEC mask around the whole loop --
      // not a select per load (measured in round 1: that serialised the eight loads in flight) -- and the masked lanes' loads
      // are simply not issued: 19 % less L2 traffic.
      const int lanes_on = min(64, ((P - chunk * 1024 + 15) >> 4) + 1);
      const uint64_t lanes_mask = lanes_on >= 64 ? ~0ull : (1ull << lanes_on) - 1ull;
      // behind this modality's last group the next modality's first is requested (whether or not that one then runs)
      auto next_begin = [&]() { return m + 1 < FL_MAX_MODALITIES ? (int)field(11 + 3 * (m + 1)) : off_begin; };
      // The group after the one in work is requested before that one's vector loads are waited for: a group costs one memory
      // round trip, not two.  Past a bank's last group this reads the table's FL_SCAN_OFF_PAD entries; an offset beyond
      // n_pad is never turned into a load.
      uint32_t nxt = 0;
      auto request = [&](int at) { return a.offs[at + l7]; };
      {
        // One piece: N features from offset S0 of `ov` on -- those behind the group's eighth from `ov2`, the group after it --
        // under one EXEC region: the lanes that are alive and their upper neighbours, of those this modality has positions
        // for.  The first eight loads are issued at once; load 8 + u is issued when load u has been added, into the registers
        // that one leaves, so a long piece keeps eight loads in flight and the load registers stay 32.  No branch stands
        // between the loads of a piece.
        // TAIL: lane 63 loads, and its bytes 16..19 have no upper neighbour to come from.  Lane f of the wave then fetches
        // the dword behind lane 63's sixteen bytes of the feature at offset f -- ONE vector load in front of the piece's
        // feature loads (vector loads return in order), taken apart with v_readlane and a select when the feature is
        // added.  The addresses are all over the linear memories; as one scalar load per feature they were misses of the
        // scalar cache, sixteen per item, and sixteen address pairs and results in scalar registers.  They are needed only
        // where lane 63 loads at all: not for a template whose positions end below the chunk's last lane (52 lanes of a
        // bench template), nor once lane 63 is dead.  Elsewhere the lane the DPP has no source for takes a zero.
        auto piece = [&](auto s0_, auto n_, auto tail_, const uint32_t ov2, const uint32_t tv) {
          constexpr int S0 = decltype(s0_)::value, N = decltype(n_)::value, InFlight = N < 8 ? N : 8;
          constexpr bool TAIL = decltype(tail_)::value != 0;
          uint4 v[InFlight];
          unsigned mis_all = 0;                            // the misalignments, two bits each: one scalar register
          auto issue = [&](const int u) {
            unsigned off = rl(S0 + u < 8 ? ov : ov2, (S0 + u) & 7);
            // (a streamed load waits for the sums of the one whose registers it takes: without this the compiler issues the
            // piece's loads all at once, into twice the registers.  The tie is on the scalar offset, not on the vector register
            // it is read from: a copy of that one made under the piece's EXEC would leave out the dead lanes it is read from.)
            if (u >= InFlight) asm("" : "+s"(off) : "v"(a0), "v"(a1), "v"(a2), "v"(a3));
            const unsigned mis_u = (lm_mis + off) & 3u;
            mis_all |= mis_u << (2 * u);
            // buffer_load ... v_lane_off, s[rsrc], s_feature_off offen: the lane's byte offset is one loop-invariant VGPR and
            // the feature's offset a scalar operand -- no per-lane 64-bit address arithmetic (it was 2 of the 10 VALU
            // instructions per feature)
            const u32x4 ld = __builtin_amdgcn_raw_buffer_load_b128(rsrc, lane_off, off - mis_u + 4u, 0);   // 4-byte aligned
            v[u % InFlight] = make_uint4(ld.x, ld.y, ld.z, ld.w);
          };
          auto take = [&](const int u) {
            const unsigned mis_u = (mis_all >> (2 * u)) & 3u;
            const uint4 x = v[u % InFlight];
            uint32_t e = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x.x, 0x130, 0xF, 0xF, true);        // wave_shl:1
            if (TAIL) {
              const uint32_t t = rl(tv, S0 + u);           // (read for the wave, then selected: no branch)
              e = lane == 63 ? t : e;
            }
            a0 += __builtin_amdgcn_alignbyte(x.y, x.x, mis_u);
            a1 += __builtin_amdgcn_alignbyte(x.z, x.y, mis_u);
            a2 += __builtin_amdgcn_alignbyte(x.w, x.z, mis_u);
            a3 += __builtin_amdgcn_alignbyte(e, x.w, mis_u);
          };
#pragma unroll
          for (int u = 0; u < InFlight; ++u) issue(u);
#pragma unroll
          for (int u = 0; u < N; ++u) {
            take(u);
            if (u + InFlight < N) issue(u + InFlight);
          }
        };
        auto add_features = [&](auto s0_, auto n_, const uint32_t ov2) {
          constexpr int S0 = decltype(s0_)::value, N = decltype(n_)::value;
          const uint64_t need = (alive | alive << 1) & lanes_mask;
          FL_SCAN_STAT(1, N);
          FL_SCAN_STAT(2, N * __builtin_popcountll(need));
          const bool tail_on = (need >> 63) != 0ull;   // wave-uniform
          // (by lanes S0 .. S0 + N - 1 whether or not they are alive.  A first piece above eight takes lanes 8 .. 15's addresses
          // from `ov2`, the request just issued, and so waits for it in front of the piece: a round trip only a launch in
          // which lane 63 loads pays; not measured apart, profiles/README.md)
          uint32_t tv = 0;
          if (tail_on && (unsigned)(lane - S0) < (unsigned)N) {
            const uint32_t of = lane < 8 ? ov : ov2;
            tv = __builtin_amdgcn_raw_buffer_load_b32(rsrc, of - ((lm_mis + of) & 3u) + 4u + 1024u, 0, 0);
          }
          if (__builtin_amdgcn_inverse_ballot_w64(need)) {
            if (tail_on) piece(s0_, n_, ScanInt<1>{}, ov2, tv);
            else piece(s0_, n_, ScanInt<0>{}, ov2, tv);
            if (S0 == 0) asm volatile("" :: "v"(nxt));     // (keeps the request above in front of this group's loads)
          }
          f_done += N;
        };
        // the same bound inside the modality, `done` of its (padded) features in: the lane's largest byte so far on top of its
        // largest finished total (an over-estimate of its largest partial total, so nothing reachable is ever dropped)
        auto reachable = [&](int done, [[maybe_unused]] bool first_piece) {
          const u16x2 b0 = pk_bytes_max(a0), b1 = pk_bytes_max(a1), b2 = pk_bytes_max(a2), b3 = pk_bytes_max(a3);
          const u16x2 bm = __builtin_elementwise_max(__builtin_elementwise_max(b0, b1), __builtin_elementwise_max(b2, b3));
          const int part = (int)max(bm.x, bm.y);
          const int left = nf_all - nf + max(0, h_nf - done);
          // (every live lane votes: one past this modality's template_positions adds nothing here, its bound is simply
          // generous -- it may still collect from a modality whose template_positions reach further)
          if (still((int)mx_tot + part + 4 * left > prune_threshold)) return true;                // wave-uniform
          FL_SCAN_STAT(4 + f_done, 1);
          if (first_piece) FL_SCAN_STAT(FL_SCAN_STATS_N - 1, 1);
          return false;
        };
        // A modality's first piece has no check inside: FIRST features where the modality has a second group, its first eight
        // where it has not.  No item of the bench bank ends before its ninth feature, so the check behind eight only costs a
        // round trip; 16 end nearly every item after ONE round trip and are the slowest, because every lane then loads what the
        // checks at 12 and 14 would have spared most of them: 12 measure best (profiles/README.md).  Its check, and those of the
        // rest of that group, go by the bit of the group that holds feature FIRST - 1.  Behind it the pieces end at the multiples of STEP; bit g of
        // `mid` enables the checks inside and at the end of group g.
        int k = 0;
        if (n_pad > 0) {
          if (o_at != off_begin) ov = request(off_begin);  // rare: the modality before this one added nothing in this chunk
          const int nxt_at = 8 < n_pad ? off_begin + 8 : next_begin();
          nxt = request(nxt_at);
          if (FIRST > 8 && n_pad > 8) {
            const int nx2_at = 16 < n_pad ? off_begin + 16 : next_begin();   // the group behind the two this piece reads
            const uint32_t nx2 = request(nx2_at);
            add_features(ScanInt<0>{}, ScanInt<FIRST>{}, nxt);
            asm volatile("" :: "v"(nx2));
            if (flag(2u) && !reachable(FIRST, true)) return;
            ov = nxt;
            if (FIRST == 12 && STEP == 2) {
              add_features(ScanInt<4>{}, ScanInt<2>{}, 0u);
              if (flag(2u) && !reachable(14, false)) return;
            } else if (FIRST == 12) {
              add_features(ScanInt<4>{}, ScanInt<4>{}, 0u);
              if (flag(2u) && !reachable(16, false)) return;
            }
            if (FIRST == 14 || (FIRST == 12 && STEP == 2)) {
              add_features(ScanInt<6>{}, ScanInt<2>{}, 0u);
              if (flag(2u) && !reachable(16, false)) return;
            }
            ov = nx2;
            o_at = nx2_at;
            k = 16;
          } else {
            add_features(ScanInt<0>{}, ScanInt<8>{}, 0u);
            if (flag(1u) && !reachable(8, true)) return;
            ov = nxt;
            o_at = nxt_at;
            k = 8;
          }
        }
        for (; k < n_pad; k += 8) {
          const int at = off_begin + k;
          if (o_at != at) ov = request(at);
          const int nxt_at = k + 8 < n_pad ? at + 8 : next_begin();
          nxt = request(nxt_at);
          const bool chk = flag(1u << (k >> 3));           // wave-uniform (k < 64: a bit of the mask)
          if (STEP == 8) {
            add_features(ScanInt<0>{}, ScanInt<8>{}, 0u);
            if (chk && !reachable(k + 8, false)) return;
          } else if (STEP == 4) {
            add_features(ScanInt<0>{}, ScanInt<4>{}, 0u);
            if (chk && !reachable(k + 4, false)) return;
            add_features(ScanInt<4>{}, ScanInt<4>{}, 0u);
            if (chk && !reachable(k + 8, false)) return;
          } else {
            add_features(ScanInt<0>{}, ScanInt<2>{}, 0u);
            if (chk && !reachable(k + 2, false)) return;
            add_features(ScanInt<2>{}, ScanInt<2>{}, 0u);
            if (chk && !reachable(k + 4, false)) return;
            add_features(ScanInt<4>{}, ScanInt<2>{}, 0u);
            if (chk && !reachable(k + 6, false)) return;
            add_features(ScanInt<6>{}, ScanInt<2>{}, 0u);
            if (chk && !reachable(k + 8, false)) return;
          }
          ov = nxt;
          o_at = nxt_at;
        }
      }
      const uint32_t acc[4] = {a0, a1, a2, a3};
      const int nv = P - j0;                          // the lane's positions below template_positions: cells >= it stay 0 (:1160)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c = nv - 4 * q;                     // ... of them in word q
        const uint32_t w = acc[q] & (c >= 4 ? ~0u : c <= 0 ? 0u : (1u << (8 * c)) - 1u);
        tp[2 * q] += w & 0x00FF00FFu;
        tp[2 * q + 1] += (w >> 8) & 0x00FF00FFu;
      }
    }
    // (the pyramid's index is read from the record again where it is needed: the record stays in its vector register)
    const int g_end = (int)field(8);
    if (flag(F_TAPPED)) {
      const FL_CONST_AS ScanArgs *kr = kargs();
      const int WH = kr->WH;
      uint16_t *d = kr->dbg + ((size_t)frame * (unsigned)kr->dbg_count + (g_end - kr->dbg_first)) * WH;
#pragma unroll
      for (int i = 0; i < 16; ++i)
        if (j0 + i < WH) d[j0 + i] = (uint16_t)tot_at(i);
    }
    // coarse threshold (linemod.cpp:1483-1506), float expression evaluated as written
    const int raw_threshold = (int)(2 * nf + thr100 * (2 * nf) + 0.5f);
    const uint32_t mx = tot_max();
    FL_SCAN_STAT(3, 1);
    if ((int)mx <= raw_threshold || !__builtin_amdgcn_inverse_ballot_w64(alive)) return;   // dead lanes emit nothing (see `alive`)
    const FL_CONST_AS ScanArgs *kr = kargs();
    const int W = kr->W, WH = kr->WH, T = kr->T, cap = kr->cap;
    uint8_t *ws = kr->ws + (size_t)frame * kr->ws_stride;
    int *count = (int *)(ws + kr->off_count);
    FlCand *cand = (FlCand *)(ws + kr->off_cand);
    const int offset = T / 2 + (T % 2 - 1);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int raw = (int)tot_at(i);
      const int j = j0 + i;
      if (raw > raw_threshold && j < WH) {
        const int rr = j / W, c = j - rr * W;
        const int idx = atomicAdd(count, 1);
        if (idx < cap) {
          FlCand cd;
          cd.x = c * T + offset;
          cd.y = rr * T + offset;
          cd.g = g_end;
          cd.sim = (raw * 100.f) / (4 * nf) + 0.5f;                               // :1502
          cand[idx] = cd;
        }
      }
    }
  };

  const int it_end = min(a.n_items, it + a.run * a.item_step);
  for (;;) {
    const uint32_t cur = rec;
    const bool cur_on = ((rl(cur, 16) >> ((it & 3) * 8)) & 0xFFu) != 0;   // wave-uniform: matchClass is not called for a class left out
    // the next item's record and flag are requested before this item's loads (behind the last item: its own again)
    const int nx = it + a.item_step;
    const bool more = nx < it_end;
    const int nxc = more ? nx : it;
    rec = request_item(nxc);
    if (cur_on) scan_item(cur);
    if (!more) break;
    it = nx;
  }
}

// ------------------------------------------------------------------------------------------
// Work items a wave of k_scan walks: FL_SCAN_RUN_AUTO where the launch then still has FL_SCAN_FILL times the waves the device
// holds at once, else half of that, and so on down to 1 (so the small-batch launches are what they were: one frame of 2000
// templates is 2000 items for 1024 SIMDs).  Option scan_run != 0 forces a length.
#ifndef FL_SCAN_RUN_AUTO
#define FL_SCAN_RUN_AUTO 8
#endif
#define FL_SCAN_FILL 4
#define FL_SCAN_FILL_WAVES 6      // (the pruned scan's waves per SIMD when the run lengths were measured: the small batches keep them)
static int fl_scan_run(const fl_context *ctx, int items, int n_frames)
{
  if (ctx->opt.scan_run) return (int)ctx->opt.scan_run;
  const long need = (long)FL_SCAN_FILL * ctx->cus * 4 * (ctx->opt.scan_prune ? FL_SCAN_FILL_WAVES : FL_SCAN_WPE);
  int run = FL_SCAN_RUN_AUTO;
  while (run > 1 && (long)n_frames * ((items + run - 1) / run) < need) run /= 2;
  return run;
}

// Feature loads between two of k_scan's checks behind a modality's first eight (the STEP the kernel is built for).  A finer step
// trades a dependent round trip for load instructions not issued, which pays where the launch keeps every CU's vector memory
// path busy: from FL_SCAN_STEP_FRAMES frames on (measured at 256 and 4096); below, where an item costs its round trips and
// nothing else, groups of eight (the scan of 1 and of 64 frames: 0.017 against 0.020 ms, 0.111 against 0.113 ms,
// profiles/README.md).  Option scan_prune_step != 0 forces a step.
#ifndef FL_SCAN_STEP_FRAMES
#define FL_SCAN_STEP_FRAMES 256
#endif
static int fl_scan_step(const fl_context *ctx, int n_frames)
{
  if (ctx->opt.scan_prune_step) return (int)ctx->opt.scan_prune_step;
  return n_frames >= FL_SCAN_STEP_FRAMES ? FL_SCAN_STEP : 8;
}

// Features of a modality's first piece (the FIRST the kernel is built for).  A longer piece pays where the check behind eight
// features ends no item: where a position may lose more than seven features' worth of points (4 nf - raw_threshold > 28, from
// the bank's typical feature count and the call's threshold), so that only a lane that has scored next to nothing goes there.
// Measured both ways (profiles/README.md): the 62-feature bench bank at 75 % may lose 31 points and gains 5 % with 12; the
// 30-feature coarsest level of the three-level bank may lose 15, most of its items end behind eight features, and 12 cost it
// 20 % of the scan.  The boundary at 28 lies between these two measured points and has not been measured itself.
// FL_SCAN_FIRST from FL_SCAN_STEP_FRAMES frames on, eight below.  Option scan_first != 0 forces a length.
#ifndef FL_SCAN_FIRST
#define FL_SCAN_FIRST 12
#endif
static int fl_scan_first(const fl_detector *det, int n_frames, float threshold)
{
  const fl_context *ctx = det->ctx;
  if (ctx->opt.scan_first) return (int)ctx->opt.scan_first;
  const int nf = det->scan_nf_typical;
  const int raw_threshold = (int)(2 * nf + threshold / 100.f * (2 * nf) + 0.5f);
  return n_frames >= FL_SCAN_STEP_FRAMES && 4 * nf - raw_threshold > 28 ? FL_SCAN_FIRST : 8;
}

// The scan of n_frames frames' coarsest level into their candidate buffers.  dbg (fl_similarity_maps): the raw maps of
// pyramids [dbg_first, dbg_first + dbg_count) of every frame, else null.
int fl_launch_scan(fl_detector *det, int n_frames, float threshold, uint16_t *dbg, int dbg_first, int dbg_count)
{
  fl_context *ctx = det->ctx;
  const int M = det->M;
  const FlLevelGeom &g = det->geom[det->L - 1];
  ScanArgs a;
  a.offs = det->d_scan_off;
  a.enabled = det->d_item_enabled;
  a.ws = det->d_ws;
  a.ws_stride = det->ws_stride;
  for (int m = 0; m < FL_MAX_MODALITIES; ++m) a.lm_off[m] = g.lm_off[m < M ? m : 0];
  a.off_count = det->off_count;
  a.off_cand = det->off_cand;
  a.M = M;
  a.W = g.W;
  a.WH = g.WH;
  a.T = g.T;
  a.cap = det->cap;
  a.threshold = threshold;
  a.prune = ctx->opt.scan_prune != 0;                   // development switches (fl_context_set_option)
  a.prune_mid = ctx->opt.scan_prune_mid >= 0 ? (unsigned)ctx->opt.scan_prune_mid : FL_SCAN_PRUNE_MID;
  a.prune_lanes = ctx->opt.scan_prune_lanes != 0;
  a.dbg = dbg;
  a.dbg_first = dbg_first;
  a.dbg_count = dbg ? dbg_count : 0;
  a.items = det->d_scan_items;
  a.n_items = det->n_scan_items;
  const int items = det->n_scan_items;
  if (items <= 0) return FL_OK;
  a.run = fl_scan_run(ctx, items, n_frames);
  const int waves = (items + a.run - 1) / a.run;      // per frame
  a.bpf = (waves + 3) / 4;
  a.wave_step = 1;                                    // wave w: items w, w + 4 bpf, ...: the trained views, which lead the bank
  a.item_step = a.bpf * 4;                            // and never prune, are spread over the frame's waves
  a.n_frames = n_frames;
  dim3 grid((unsigned)(a.bpf * ((n_frames + 7) / 8) * 8));
  // the pruned builds by [STEP 2, 4, 8][FIRST 8, 12, 14, 16]; a value outside takes 8
  typedef void (*ScanKernel)(ScanArgs);
  constexpr int P = FL_SCAN_WPE_PRUNED;
  static const ScanKernel pruned[3][4] = {{k_scan<P, 2, 8>, k_scan<P, 2, 12>, k_scan<P, 2, 14>, k_scan<P, 2, 16>},
                                          {k_scan<P, 4, 8>, k_scan<P, 4, 12>, k_scan<P, 4, 14>, k_scan<P, 4, 16>},
                                          {k_scan<P, 8, 8>, k_scan<P, 8, 12>, k_scan<P, 8, 14>, k_scan<P, 8, 16>}};
  const int step = fl_scan_step(ctx, n_frames), first = fl_scan_first(det, n_frames, threshold);
  const ScanKernel kern = !a.prune ? k_scan<FL_SCAN_WPE, 8, 8>
                                   : pruned[step == 2 ? 0 : step == 4 ? 1 : 2][first == 12 ? 1 : first == 14 ? 2 : first == 16 ? 3 : 0];
  hipLaunchKernelGGL(kern, grid, dim3(256), 0, ctx->stream, a);
  FL_HIP(ctx, hipGetLastError());
#ifdef FL_SCAN_STATS
  {
    unsigned long long st[FL_SCAN_STATS_N], zero[FL_SCAN_STATS_N] = {0};
    FL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    FL_HIP(ctx, hipMemcpyFromSymbol(st, HIP_SYMBOL(d_scan_stats), sizeof(st)));
    FL_HIP(ctx, hipMemcpyToSymbol(HIP_SYMBOL(d_scan_stats), zero, sizeof(zero)));
    fprintf(stderr, "k_scan: %d frames, %llu items, %.2f feature loads and %.1f lane-loads per item, %llu items to their end; ended "
            "by a first piece's check %llu; after f features:", n_frames, st[0], st[0] ? (double)st[1] / st[0] : 0.0,
            st[0] ? (double)st[2] / st[0] : 0.0, st[3], st[FL_SCAN_STATS_N - 1]);
    for (int f = 0; f + 5 < FL_SCAN_STATS_N; ++f)
      if (st[4 + f]) fprintf(stderr, " %d: %llu", f, st[4 + f]);
    fprintf(stderr, "\n");
  }
#endif
  return FL_OK;
}
