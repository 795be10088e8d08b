// The s-step cycle's dispatch as plain host arithmetic: which sweeps and scalar launches build each block of a restart cycle,
// in which form and on which grid. nk_ss_cycle (nk_sstep.hip) waits for progress, asks ss_plan_block for the next block and
// runs what comes back; nothing here touches the device, so a host compiler builds it and tests/test_ss_plan.py walks every
// combination of forms. What the forms ARE is told where the kernels are (nk_sstep.hip); operator launches are not planned
// (whether the resident matrix-powers kernel takes a block is decided when it is launched).
#pragma once

#include <cassert>
#include <cstdint>
#include <cstdlib>

constexpr int SS_R = 256;        // rows per tile = threads per workgroup
constexpr int SS_MAX_WG_PER_CU = 4;
// what a scalar launch of the block scheme (k_ss_job) does
constexpr int SSJ_F1 = 1, SSJ_F2 = 2, SSJ_HESS = 4, SSJ_BACK = 8, SSJ_COEF2 = 16, SSJ_PREP = 32;

// ----------------------------------------------------------------------------- the A/B switches, read from the environment once
struct ss_switches {
  bool fused = true;        // NK_SS_FUSED=0: reduction, all-reduce and k_ss_tail1/2 as launches of their own, no scalar work inside sweeps
  int per_cu = 0;           // NK_SS_PER_CU=p: p persistent workgroups per CU (≤ 4) instead of what the runtime says a CU holds
  bool grid_a = true;       // NK_SS_GRID_A=0: sweep A of the default shapes takes sweep B's grid, not one workgroup per CU
  int grid_a_host = 0;      // NK_SS_GRID_A_HOST=1: a sweep A that hosts Hessenberg work gets a 257th workgroup for it
  bool kconst = true;       // NK_SS_KCONST=0: no compile-time-k instances for the default cycle's shapes (nor what builds on them)
  bool ro = true;           // NK_SS_RO=0: a sweep B that stores nothing runs the staging kernel, not the read-only one
  bool ro_grid = true;      // NK_SS_RO_GRID=0: the read-only sweep B keeps two workgroups per CU
  bool barriers = false;    // NK_SS_BARRIERS=1: the Gram phase's wavefronts wait for each other at workgroup barriers again
  bool mm = true;           // NK_SS_MM=0: sweep B of the default shapes without the matrix-core update (k_ss_block_mm)
  bool implicit = true;     // NK_SS_IMPLICIT=0: every block but the last gets its third sweep
  bool last_sweep = false;  // NK_SS_LAST_SWEEP=1: the cycle's last block is treated like any other
  bool host_a = true;       // NK_SS_HOST_A=0: the first block is closed by a launch of its own, not by workgroups of the second's sweep A
  int host_a_wgs = 20;      // NK_SS_HOST_A_WGS=w: that many workgroups (1..64; 240 entries: three rounds of 4 × 20 wavefronts — 8 left the job longer than the sweep, 30 cost the sweep)
  bool host_b = true;       // NK_SS_HOST_B=0: sweep B hosts nobody's Hessenberg work
  bool defer = true;        // NK_SS_DEFER=0: a block's second factorisation in a launch of its own (round 4's cycle)
  bool tail_back = true;    // NK_SS_TAIL_BACK=0: the back-substitution as a launch of its own (k_backsolve)
  int defer_hess = -1;      // NK_SS_DEFER_HESS=0 / 1: the pending block's Hessenberg work in the job / hosted by sweep B, whatever the protocol
  bool nostore = true;      // NK_SS_NOSTORE=0: sweep B of the cycle's last block stores its columns
};
inline ss_switches ss_switches_from_env() {
  const auto num = [](const char *name, int unset) { const char *v = std::getenv(name); return v ? std::atoi(v) : unset; };
  ss_switches w;
  w.fused = num("NK_SS_FUSED", 1) != 0;
  w.per_cu = num("NK_SS_PER_CU", 0);
  w.grid_a = num("NK_SS_GRID_A", 1) != 0;
  w.grid_a_host = num("NK_SS_GRID_A_HOST", 0);
  w.kconst = num("NK_SS_KCONST", 1) != 0;
  w.ro = num("NK_SS_RO", 1) != 0;
  w.ro_grid = num("NK_SS_RO_GRID", 1) != 0;
  w.barriers = num("NK_SS_BARRIERS", 0) != 0;
  w.mm = num("NK_SS_MM", 1) != 0;
  w.implicit = num("NK_SS_IMPLICIT", 1) != 0;
  w.last_sweep = num("NK_SS_LAST_SWEEP", 0) != 0;
  w.host_a = num("NK_SS_HOST_A", 1) != 0;
  w.host_a_wgs = num("NK_SS_HOST_A_WGS", 20);
  w.host_a_wgs = w.host_a_wgs < 1 ? 1 : (w.host_a_wgs > 64 ? 64 : w.host_a_wgs);
  w.host_b = num("NK_SS_HOST_B", 1) != 0;
  w.defer = num("NK_SS_DEFER", 1) != 0;
  w.tail_back = num("NK_SS_TAIL_BACK", 1) != 0;
  w.defer_hess = num("NK_SS_DEFER_HESS", -1);
  w.nostore = num("NK_SS_NOSTORE", 1) != 0;
  return w;
}
inline const ss_switches &ss_env_switches() {   // the process's switches: every launch helper and every cycle sees the same ones
  static const ss_switches w = ss_switches_from_env();
  return w;
}

// ----------------------------------------------------------------------------- what a cycle's decisions depend on
// workgroups of sweep `mode` (0/1/2 = A/B/C) for a block of s columns behind k that a CU holds at once
typedef int (*ss_occupancy_fn)(void *user, int mode, int k, int s);
struct ss_cycle_cfg {
  int steps = 0, s = 0;          // Arnoldi steps of the cycle, block size
  int64_t n = 0, ldv = 0;
  bool v_aligned16 = false;      // the basis starts on a 16-byte boundary
  int num_cus = 0;
  bool single_rank = true, peer_ok = true;   // peer_ok: one rank, or peer-mapped arenas that take two partial blocks in one message
  bool newton = false;           // Newton-basis blocks
  bool auto_grow = false;        // automatic block sizes of a solve that stops on a tolerance: 4, 8, 15 … / 2, 4, 6 …
  bool fixed_work = false;       // nothing can stop the cycle early
  bool accepts_back = false;     // the caller lets the cycle's last scalar launch back-substitute
  bool audit_on = false;         // (development) the audit wants every block's columns in memory
  int nblk_slots = 0, nfix = 0;  // factor slots of the workspace; capacity of the list of blocks left at their first pass (NK_SS_NFIX)
  ss_occupancy_fn occupancy = nullptr;
  void *occ_user = nullptr;
};

// ----------------------------------------------------------------------------- shape predicates and grids
// size class of the Gram block: k + s ≤ 16·class; 0 = the streaming form (any k + s ≤ 80)
inline int ss_class(int k, int s) { return k + s <= 16 ? 1 : (k + s <= 32 ? 2 : (k + s <= 48 ? 3 : 0)); }
// widths the sweeps are compiled for; any other block is cut into these (the last block of a cycle, odd block sizes)
inline int ss_block_width(int want) {   // (round 6: 3, 5, 7, 10 and 12 left the list — 45 % of the sweep instantiations for ragged tails only)
  if (want >= 15) return 15;
  if (want >= 8) return 8;
  if (want >= 6) return 6;
  if (want >= 4) return 4;
  return want >= 2 ? 2 : 1;
}
inline bool ss_fusable(const ss_switches &sw, int k, int s) { return sw.fused && ss_class(k, s) != 0; }
// persistent workgroups per CU = what the runtime says a CU holds of the instance that will run (LDS tile and register
// footprint: 190–196 VGPRs for the Gram sweeps of a 15-column block behind 16 columns — two workgroups, not the three a table
// of size classes once said; the third of every CU ran as a second round on a third of the chip)
inline int ss_per_cu(const ss_cycle_cfg &c, const ss_switches &sw, int k, int s) {
  if (sw.per_cu > 0) return sw.per_cu > SS_MAX_WG_PER_CU ? SS_MAX_WG_PER_CU : sw.per_cu;
  const int a = c.occupancy(c.occ_user, 0, k, s), b = c.occupancy(c.occ_user, 1, k, s);
  const int per_cu = a < b ? a : b;
  return per_cu < 1 ? 1 : (per_cu > SS_MAX_WG_PER_CU ? SS_MAX_WG_PER_CU : per_cu);
}
inline int ss_ntiles(const ss_cycle_cfg &c) { return (int)((c.n + SS_R - 1) / SS_R); }
// Workgroups of a sweep: as many per CU as fit — but not more than divide the tiles evenly. A workgroup walks ⌈tiles / grid⌉
// tiles, so a CU is busy for per_cu·⌈tiles / (CUs·per_cu)⌉ of them: with 4096 tiles (n = 2²⁰) on 256 CUs three workgroups per CU
// (what the 15-column block behind one column fits) make that 18 where two or four make it 16 — measured 25.6 → 24.2 and
// 47.4 → 45.7 µs for sweeps A and B of that shape with two. The largest count that reaches the minimum is taken.
inline int ss_grid(const ss_cycle_cfg &c, const ss_switches &sw, int k, int s) {
  const int ntiles = ss_ntiles(c);
  const int occ = ss_per_cu(c, sw, k, s);
  int best = occ;
  int64_t best_cost = INT64_MAX;
  for (int p = occ; p >= 1; --p) {
    const int64_t g = (int64_t)c.num_cus * p;
    const int64_t cost = (int64_t)p * ((ntiles + g - 1) / g);
    if (cost < best_cost) { best_cost = cost; best = p; }
  }
  int g = c.num_cus * best;
  if (g > ntiles) g = ntiles;
  return g > 0 ? g : 1;
}
// Sweep A (read-only) of the default cycle's shapes runs ONE workgroup per CU — measured on the same box, stand-alone:
// 24.1 → 22.0 µs behind one column, 45.9 → 42.1 µs behind 16 (6.1–6.2 TB/s; the writing sweep B gains nothing from it). When it
// hosts the previous block's Hessenberg work the hosting workgroup is one of these (it streams nothing and has a CU to itself:
// 49 µs; as a 257th workgroup beside a streaming one 54 µs, inside a grid of 512 52 µs — the hosted scalar work, ≈ 45 µs under
// load against 29 µs as a launch of its own, is what that launch waits for, not its 255 streaming workgroups).
// Other shapes: the grid of sweep B.
inline int ss_grid_a(const ss_cycle_cfg &c, const ss_switches &sw, int k, int s, bool hosting) {
  if (!sw.grid_a || !sw.kconst || s != 15 || (k != 1 && k != 16) || ss_ntiles(c) < 2 * c.num_cus) return ss_grid(c, sw, k, s);
  return c.num_cus + (hosting ? sw.grid_a_host : 0);
}
// Sweep B that stores nothing takes the read-only kernel (k_ss_block_ro): behind 16 columns, 32-bit byte offsets over the whole
// basis, 16-byte row pairs
inline bool ss_b_read_only(const ss_switches &sw, int64_t ldv, bool v_aligned16, int k, int s) {
  return sw.ro && k == 16 && s == 15 && (int64_t)(k + s) * ldv * 8 < ((int64_t)1 << 32) - 8 && (ldv & 1) == 0 && v_aligned16;
}
// Sweep B of this shape can host a Hessenberg workgroup (the matrix-core form of the default cycle's shapes)
inline bool ss_b_can_host(const ss_switches &sw, int64_t ldv, int k, int s) {
  return sw.host_b && sw.mm && s == 15 && (k == 1 || k == 16) && (int64_t)s * ldv * 8 < ((int64_t)1 << 32) - 8;
}
// Sweep A of this shape can host the scalar launch that closes the previous block in extra workgroups (k_ss_block's JOBHOST
// instance: the compile-time-k form of the default cycle's second block). One rank only: a hosted job cannot wait for peers
// while the streaming workgroups of its own launch hold the chip.
// The job's workgroups take the place of streaming ones (the sweep's LDS tile admits two workgroups per CU and the grid fills
// them: workgroups added to a full grid start when the sweep is over).
inline bool ss_a_can_host_job(const ss_switches &sw, bool single_rank, int k, int s) {
  return sw.host_a && sw.kconst && single_rank && s == 15 && k == 16 && ss_class(k, s) == 2;
}

// ----------------------------------------------------------------------------- the plan of a block
// Implicit second pass (ss_switches::implicit): a block that is not the cycle's last is left at its first pass as well —
// no sweep C; the next blocks carry their Gram products through its (C₂, R₂) (ss_fix_to_true / _to_stored), its Hessenberg
// columns are a launch of their own, the back-substitution adapts y block by block. One sweep over k + 2s columns less per block.
// Blocks are left at their first pass with the NEWTON basis only (monomial blocks of 6–8 columns live near the rank-loss bar
// and keep the explicit second update), and only while the first pass leaves them NEARLY orthonormal: the Hessenberg recovery
// of the next block starts from a stored column, a combination u of true basis vectors whose images carry this block's
// recovery errors — harmless for u ≈ e_k, amplified column by column when pass 1 was far off (a block within a factor of ≈ 30
// of losing rank: oracle, Arnoldi residual 5e-2 against 1e-7 for the explicit update at a departure of 0.75, equal up to 0.2).
// ss_first_pass_departure measures max(|C₂|, |R₂ − I|) in the reduction's tail; above 0.1 the block counts as broken and
// takes the fall-back (narrower blocks), exactly like a lost pivot.
inline bool ss_implicit_mode(const ss_cycle_cfg &c, const ss_switches &sw) { return sw.implicit && c.newton; }
// The deferred second factorisation: with the implicit second pass on the fused path. Several ranks: the fused scalar launches
// are also the all-reduce — on peer-mapped arenas only.
inline bool ss_deferred(const ss_cycle_cfg &c, const ss_switches &sw) {
  return sw.defer && ss_implicit_mode(c, sw) && c.peer_ok && ss_fusable(sw, 1, 1);
}

// loop-carried between the blocks of a cycle
struct ss_cycle_state {
  int k = 1;              // orthonormal columns so far (column 0 = r₀, un-normalised)
  int blk = 0;            // index of the next block within the cycle = its slot of pass-2 factors
  int grow = 0, prev_sb = 0;   // width cap of the next block (automatic sizes double); width of the block before it
  int nfix = 0;           // blocks left at their first pass so far (the list the back-substitution walks)
  struct { bool on; int k, sb, grid; } dp = {false, 0, 0, 0};   // deferred: sweep B has run, the second factorisation has not (grid: its partial sums per entry)
  struct { int k, sb; } pend = {0, 0};   // its Hessenberg columns wait for a sweep A to host them (sb = 0: nobody's do)
  int prev_k0 = 0, prev_sb2 = 0;         // the previous block if it was left at its first pass (prev_sb2 = 0: it was not)
  bool raw_on = false;    // the last block's sweep B stored nothing: the closing launch must back-substitute
};
inline ss_cycle_state ss_plan_begin(const ss_cycle_cfg &c) {
  ss_cycle_state st;
  // A solve that stops on a tolerance may need 2 iterations or 200: a block's operator applications past the column that meets
  // the tolerance are wasted (a multigrid V-cycle each, under that preconditioner). Automatic block sizes therefore start small
  // in every cycle and double — 4, 8, 15, 15 … with the Newton basis, 2, 4, 6, 6 … with the monomial one —: a solve that needs
  // k iterations applies the operator < 2k times, and one that fills the cycle builds most of it in full-width blocks. The
  // fixed-work protocol and explicit block sizes take full blocks from the start.
  st.grow = c.auto_grow ? (c.newton ? 4 : 2) : c.s;
  st.prev_sb = c.s;
  return st;
}
inline bool ss_plan_more(const ss_cycle_cfg &c, const ss_cycle_state &st) { return st.k - 1 < c.steps; }

enum ss_op { SS_SWEEP_A, SS_SWEEP_B, SS_SWEEP_C, SS_JOB, SS_TAIL1, SS_TAIL2, SS_HESS };
// whose argument set a launch takes besides the block's own: the block under construction, the deferred one (ss_cycle_state::dp),
// the one whose Hessenberg columns are pending (::pend)
enum ss_who { SS_NOBODY, SS_THIS, SS_DEFERRED, SS_PENDING };
struct ss_launch {
  ss_op op;
  int grid;        // sweeps: workgroups (a sweep A that hosts a job: the streaming ones); SS_JOB with SSJ_F1, SS_TAIL1/2: partial sums per entry of this block
  int mode;        // SSJ_* bits of an SS_JOB, or of the job a sweep A hosts in host_wgs extra workgroups; else 0
  int host_wgs;
  ss_who who;      // SS_JOB: whose second pass (SSJ_F2); a sweep: whose Hessenberg work or closing job it hosts; SS_HESS: whose columns
  int wk, wsb, wgrid;   // that block's k and width (sweeps: as the kernel is told them, hosting or not), its partial sums per entry
  bool nostore;    // sweep B stores nothing
  bool raw_last;   // SSJ_BACK: … and the back-substitution takes that block's combined factors
};
constexpr int SS_PLAN_MAX = 8;   // the longest list has seven: [k_ss_hess] [closing job] A, scalar, B, scalar, C or k_ss_hess
struct ss_block_plan {
  int k, sb, blk;          // the block: sb columns behind k, slot blk (ss_plan_finish: sb = 0)
  int uk0, usb;            // the block whose last STORED column starts this block's matrix powers (usb = 0: a true basis vector does)
  bool fused;              // the scalar work rides in k_ss_job and in the sweeps
  bool last_block, implicit;   // left at its first pass as the cycle's last block / because the list has room
  bool defer_this;         // sweep A, [the deferred block's second factorisation ; this block's first], sweep B — the rest is deferred
  bool host_a, host_b;     // the deferred block is closed by extra workgroups of this sweep A / its Hessenberg work rides in this sweep B
  bool raw_last;           // this sweep B stores nothing
  int grid, grid_a, grid_b;
  bool hess_first, close_first;   // the list starts with the pending block's k_ss_hess / with the deferred block's closing job
  ss_who becomes;          // what this block is to the next one: SS_DEFERRED, SS_PENDING or SS_NOBODY
  bool joins_fix_list;     // left at its first pass: one more entry for the later reductions and the back-substitution
  bool backsolved;         // ss_plan_finish: the closing job back-substitutes
  int nl;
  ss_launch l[SS_PLAN_MAX];
};
inline ss_launch &ss_plan_add(ss_block_plan &p, ss_op op, int grid) {
  assert(p.nl < SS_PLAN_MAX);
  ss_launch &l = p.l[p.nl++];
  l = ss_launch{op, grid, 0, 0, SS_NOBODY, 0, 0, 0, false, false};
  return l;
}
inline void ss_plan_hess_of_pending(ss_block_plan &p, ss_cycle_state &st) {
  ss_launch &l = ss_plan_add(p, SS_HESS, 1);
  l.who = SS_PENDING; l.wk = st.pend.k; l.wsb = st.pend.sb;
  st.pend.sb = 0;
}
// the deferred block's second pass as set 1 of a scalar launch (or of the job a sweep A hosts)
inline void ss_plan_take_deferred(ss_launch &l, const ss_cycle_state &st, int mode) {
  l.who = SS_DEFERRED; l.wk = st.dp.k; l.wsb = st.dp.sb; l.wgrid = st.dp.grid;
  l.mode |= mode;
}
// closes the deferred block in a launch of its own: second factorisation, Wi / D, Hessenberg columns — and, at the cycle's end,
// the back-substitution
inline void ss_plan_close_deferred(ss_block_plan &p, ss_cycle_state &st, bool with_back) {
  ss_launch &l = ss_plan_add(p, SS_JOB, 0);
  ss_plan_take_deferred(l, st, SSJ_F2 | SSJ_PREP | SSJ_HESS | (with_back ? SSJ_BACK : 0));
  l.raw_last = with_back && st.raw_on;
  st.dp.on = false;
}

// The next block of the cycle (ss_plan_more says whether there is one). Widths: ≤ s, cut to what the sweeps are compiled for.
inline ss_block_plan ss_plan_block(const ss_cycle_cfg &c, const ss_switches &sw, ss_cycle_state &st) {
  ss_block_plan p = {};
  const int k = st.k;
  int sb = (c.steps - (k - 1)) < c.s ? (c.steps - (k - 1)) : c.s;
  if (st.grow < sb) sb = st.grow;
  st.grow = st.grow * 2 > c.s ? c.s : st.grow * 2;
  sb = ss_block_width(sb);
  if (k + sb > 48 && sb > 8) sb = 8;  // the streaming size class keeps its scalar workspace within the LDS
  st.prev_sb = sb;
  p.k = k; p.sb = sb; p.blk = st.blk;
  p.uk0 = st.prev_k0; p.usb = st.prev_sb2;
  p.grid = ss_grid(c, sw, k, sb);
  // fused: the block's scalar work rides in the stage-2 reduction (its last workgroup factors the reduced block and leaves
  // the update coefficients for the next sweep's scalar loads) and in sweep C (workgroup 0: the Hessenberg columns) — one
  // rank, or several on peer-mapped arenas (the reduction is then the all-reduce as well). Other transports and the
  // streaming size class (k + s > 48): reduction, all-reduce and the scalar work as launches of their own.
  p.fused = ss_fusable(sw, k, sb) && c.peer_ok;
  if (st.pend.sb > 0 && !p.fused) {   // nobody to host it: the previous block's Hessenberg columns as a launch of their own
    ss_plan_hess_of_pending(p, st);
    p.hess_first = true;
  }
  // left at its first pass (no sweep C): the cycle's last block always; any other block while the list has room — whatever
  // the transport and the size class, so that every path runs the same arithmetic (results are compared bit for bit)
  p.last_block = (k - 1 + sb >= c.steps) && !sw.last_sweep;
  p.implicit = !p.last_block && ss_implicit_mode(c, sw) && st.nfix < c.nfix - 1;
  p.defer_this = ss_deferred(c, sw) && p.fused && (p.last_block || p.implicit);
  if (st.dp.on && !p.defer_this) {   // (this block takes the older form: nobody to carry the deferred one)
    ss_plan_close_deferred(p, st, false);
    p.close_first = true;
  }
  if (p.defer_this) {
    p.grid_a = ss_grid_a(c, sw, k, sb, false);
    // the fixed-work protocol, second block of the default cycle: the deferred block is closed (reduction, second factorisation,
    // Wi / D, Hessenberg columns) by extra workgroups of THIS sweep — nothing it writes is read by the streaming ones — and the
    // launch behind the sweep only factors this block's first pass
    p.host_a = st.dp.on && p.grid_a > 4 * sw.host_a_wgs && c.fixed_work && sw.defer_hess < 0 && ss_a_can_host_job(sw, c.single_rank, k, sb);
    if (p.host_a) p.grid_a -= sw.host_a_wgs;   // (streaming workgroups: the pitch of the partial blocks)
    ss_launch &a = ss_plan_add(p, SS_SWEEP_A, p.grid_a);
    if (p.host_a) {
      ss_plan_take_deferred(a, st, SSJ_F2 | SSJ_PREP | SSJ_HESS);
      a.host_wgs = sw.host_a_wgs;
    }
    // where the deferred block's Hessenberg columns are derived: in workgroup 0 of this block's sweep B when nothing can stop
    // the cycle early (fixed work) and that sweep has the hosting form; else in the job itself (the verdict arrives before sweep B)
    p.host_b = !p.host_a && st.dp.on && p.grid > 1 && ss_b_can_host(sw, c.ldv, k, sb) && (sw.defer_hess < 0 ? c.fixed_work : sw.defer_hess == 1);
    // the last block's sweep B stores nothing where the matrix-core form runs it, the cycle's last scalar launch
    // back-substitutes, the list has room and nothing else wants the columns (development audit)
    p.raw_last = p.last_block && sw.nostore && !(p.host_b && k != 16) && ss_b_can_host(sw, c.ldv, k, sb) && sw.tail_back &&
                 c.accepts_back && !c.audit_on;
    ss_launch &j = ss_plan_add(p, SS_JOB, p.grid_a);
    j.mode = SSJ_F1;
    if (st.dp.on && !p.host_a) ss_plan_take_deferred(j, st, SSJ_F2 | SSJ_PREP | (p.host_b ? 0 : SSJ_HESS));
    // the read-only sweep runs ONE workgroup per CU where the tiles allow (as the read-only sweeps A do: stand-alone 52 → 48 µs
    // at 1024² — half the prologues and partial sums, one wavefront per SIMD on the matrix pipe)
    p.grid_b = p.grid;
    if (p.raw_last && !p.host_b && sw.ro_grid && ss_b_read_only(sw, c.ldv, c.v_aligned16, k, sb) && ss_ntiles(c) >= 2 * c.num_cus &&
        p.grid > c.num_cus)
      p.grid_b = c.num_cus;
    ss_launch &b = ss_plan_add(p, SS_SWEEP_B, p.grid_b);
    if (p.host_b) { b.who = SS_DEFERRED; b.wk = st.dp.k; b.wsb = st.dp.sb; }
    b.nostore = p.raw_last;
    if (p.raw_last) st.raw_on = true;
    st.dp.on = true; st.dp.k = k; st.dp.sb = sb; st.dp.grid = p.grid_b;
    p.becomes = SS_DEFERRED;
    p.joins_fix_list = true;
  } else {
    // sweep A (hosting the previous block's Hessenberg columns if they wait), first factorisation, sweep B, second factorisation
    const bool host_prev = st.pend.sb > 0;   // (and fused: an unfused block has flushed them above)
    p.grid_a = ss_grid_a(c, sw, k, sb, host_prev);
    p.grid_b = p.grid;
    ss_launch &a = ss_plan_add(p, SS_SWEEP_A, p.grid_a);
    a.who = host_prev ? SS_PENDING : SS_NOBODY; a.wk = st.pend.k; a.wsb = st.pend.sb;
    st.pend.sb = 0;
    if (p.fused) ss_plan_add(p, SS_JOB, p.grid_a).mode = SSJ_F1;
    else ss_plan_add(p, SS_TAIL1, p.grid_a);
    ss_plan_add(p, SS_SWEEP_B, p.grid_b).wk = st.pend.k;
    if (p.fused) {   // the block's own second factorisation: coefficients for sweep C, C₂ / R₂ for whoever derives its Hessenberg columns
      ss_launch &j = ss_plan_add(p, SS_JOB, 0);
      j.mode = SSJ_F2 | SSJ_COEF2; j.who = SS_THIS; j.wk = k; j.wsb = sb; j.wgrid = p.grid_b;
    } else
      ss_plan_add(p, SS_TAIL2, p.grid_b);
    if (!p.last_block && !p.implicit) {
      ss_plan_add(p, SS_SWEEP_C, p.grid).who = p.fused ? SS_THIS : SS_NOBODY;   // (fused: its workgroup 0 derives the block's Hessenberg columns)
    } else {
      // left at its first pass: no third sweep (k_backsolve turns y into coefficients on the columns as they are; later blocks
      // carry their Gram products through this block's factors). Its Hessenberg columns — the work of sweep C's workgroup 0,
      // or already done by k_ss_tail2 on the unfused path —: the cycle's last block as a launch of its own, any other block
      // inside the NEXT block's sweep A (which also leaves Wi, D for the reductions behind it).
      if (p.implicit && p.fused) {
        st.pend.k = k; st.pend.sb = sb;
        p.becomes = SS_PENDING;
      } else if (p.fused) {
        ss_launch &h = ss_plan_add(p, SS_HESS, 1);
        h.who = SS_THIS; h.wk = k; h.wsb = sb;
      }   // (unfused: k_ss_tail2 has derived the Hessenberg columns — and Wi, D — already)
      p.joins_fix_list = true;
    }
  }
  if (p.joins_fix_list) ++st.nfix;
  st.prev_k0 = k;
  st.prev_sb2 = p.joins_fix_list ? sb : 0;
  st.k = k + sb;
  ++st.blk;
  return p;
}
// What closes the cycle once no further block is enqueued — all `steps` are planned, or the host stopped early: the pending
// block's Hessenberg columns, the deferred block's closing job, which back-substitutes where the caller accepts it.
inline ss_block_plan ss_plan_finish(const ss_cycle_cfg &c, const ss_switches &sw, ss_cycle_state &st) {
  ss_block_plan p = {};
  p.k = st.k; p.blk = st.blk;
  if (st.pend.sb > 0) {
    ss_plan_hess_of_pending(p, st);
    p.hess_first = true;
  }
  if (st.dp.on) {
    p.backsolved = sw.tail_back && c.accepts_back;
    ss_plan_close_deferred(p, st, p.backsolved);
  }
  return p;
}
