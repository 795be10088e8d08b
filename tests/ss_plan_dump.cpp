// Host-only driver of the s-step cycle's planner (csrc/nk_ss_plan.h) for tests/test_ss_plan.py.
//   ss_plan_dump cycle key=value …   the plans of one cycle, one JSON object per line (switches: the NK_SS_* environment)
//   ss_plan_dump sweep key=value …   every configuration × every switch setting × a host that stops after any block,
//                                    checked against the invariants nk_ss_cycle's NK_REQUIREs state; prints the counts
//                                    (hold=mask: those switches stay at their defaults; grids=1: a cycle is also planned with
//                                    NK_SS_RO / NK_SS_RO_GRID off and must differ in sweep B's grid and nothing else)
#include "nk_ss_plan.h"

#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

static int g_occ = 2;
static int occupancy(void *, int, int, int) { return g_occ; }

static const char *op_name(ss_op op) {
  switch (op) {
    case SS_SWEEP_A: return "A";
    case SS_SWEEP_B: return "B";
    case SS_SWEEP_C: return "C";
    case SS_JOB: return "job";
    case SS_TAIL1: return "tail1";
    case SS_TAIL2: return "tail2";
    case SS_HESS: return "hess";
  }
  return "?";
}
static const char *who_name(ss_who w) {
  return w == SS_THIS ? "this" : (w == SS_DEFERRED ? "deferred" : (w == SS_PENDING ? "pending" : "nobody"));
}
static void print_plan(const char *what, const ss_block_plan &p, const ss_cycle_state &st) {
  std::printf("{\"what\":\"%s\",\"k\":%d,\"sb\":%d,\"blk\":%d,\"uk0\":%d,\"usb\":%d,\"fused\":%d,\"last_block\":%d,\"implicit\":%d,"
              "\"defer_this\":%d,\"host_a\":%d,\"host_b\":%d,\"raw_last\":%d,\"grid\":%d,\"grid_a\":%d,\"grid_b\":%d,"
              "\"hess_first\":%d,\"close_first\":%d,\"becomes\":\"%s\",\"joins_fix_list\":%d,\"backsolved\":%d,"
              "\"state\":{\"k\":%d,\"blk\":%d,\"nfix\":%d,\"dp_on\":%d,\"pend_sb\":%d,\"raw_on\":%d},\"launches\":[",
              what, p.k, p.sb, p.blk, p.uk0, p.usb, p.fused, p.last_block, p.implicit, p.defer_this, p.host_a, p.host_b, p.raw_last,
              p.grid, p.grid_a, p.grid_b, p.hess_first, p.close_first, who_name(p.becomes), p.joins_fix_list, p.backsolved, st.k,
              st.blk, st.nfix, st.dp.on, st.pend.sb, st.raw_on);
  for (int i = 0; i < p.nl; ++i) {
    const ss_launch &l = p.l[i];
    std::printf("%s{\"op\":\"%s\",\"grid\":%d,\"mode\":%d,\"host_wgs\":%d,\"who\":\"%s\",\"wk\":%d,\"wsb\":%d,\"wgrid\":%d,"
                "\"nostore\":%d,\"raw_last\":%d}",
                i ? "," : "", op_name(l.op), l.grid, l.mode, l.host_wgs, who_name(l.who), l.wk, l.wsb, l.wgrid, l.nostore, l.raw_last);
  }
  std::printf("]}\n");
}

static bool job_mode_ok(int mode) {   // the six instances ss_launch_job has
  return mode == SSJ_F1 || mode == (SSJ_F1 | SSJ_F2 | SSJ_PREP) || mode == (SSJ_F1 | SSJ_F2 | SSJ_PREP | SSJ_HESS) ||
         mode == (SSJ_F2 | SSJ_PREP | SSJ_HESS) || mode == (SSJ_F2 | SSJ_PREP | SSJ_HESS | SSJ_BACK) || mode == (SSJ_F2 | SSJ_COEF2);
}
struct tally { long long cycles = 0, blocks = 0, violations = 0; };
static void violation(tally &t, const char *what, const ss_cycle_cfg &c, const ss_switches &sw, const ss_block_plan &p) {
  if (t.violations++ < 10)
    std::printf("{\"violation\":\"%s\",\"steps\":%d,\"s\":%d,\"k\":%d,\"sb\":%d,\"newton\":%d,\"single\":%d,\"peer_ok\":%d,\"fixed\":%d,"
                "\"back\":%d,\"grow\":%d,\"defer\":%d,\"implicit\":%d,\"fused\":%d,\"last_sweep\":%d,\"defer_hess\":%d}\n",
                what, c.steps, c.s, p.k, p.sb, c.newton, c.single_rank, c.peer_ok, c.fixed_work, c.accepts_back, c.auto_grow, sw.defer,
                sw.implicit, sw.fused, sw.last_sweep, sw.defer_hess);
}
static void check_launches(tally &t, const ss_cycle_cfg &c, const ss_switches &sw, const ss_block_plan &p, bool raw_on_before) {
  if (p.nl < 0 || p.nl > SS_PLAN_MAX) violation(t, "launch list overflows", c, sw, p);
  for (int i = 0; i < p.nl; ++i) {
    const ss_launch &l = p.l[i];
    if ((l.op == SS_JOB || (l.op == SS_SWEEP_A && l.mode)) && !job_mode_ok(l.mode)) violation(t, "job mode without an instance", c, sw, p);
    if (l.op == SS_SWEEP_B && l.who == SS_DEFERRED && l.grid <= 1) violation(t, "hosting sweep B on one workgroup", c, sw, p);
    if (l.op == SS_JOB && !(l.mode & (SSJ_F1 | SSJ_COEF2)) && raw_on_before && !(l.mode & SSJ_BACK))
      violation(t, "unstored block closed without the back-substitution", c, sw, p);
    if (l.grid < (l.op == SS_JOB && !(l.mode & SSJ_F1) ? 0 : 1)) violation(t, "empty grid", c, sw, p);
  }
}
// equal but for the workgroups of sweep B (and the partial sums per entry that it leaves to whoever reduces them)
static bool same_but_grid_b(const ss_block_plan &p, const ss_block_plan &q) {
  bool same = p.k == q.k && p.sb == q.sb && p.blk == q.blk && p.uk0 == q.uk0 && p.usb == q.usb && p.fused == q.fused &&
              p.last_block == q.last_block && p.implicit == q.implicit && p.defer_this == q.defer_this && p.host_a == q.host_a &&
              p.host_b == q.host_b && p.raw_last == q.raw_last && p.grid == q.grid && p.grid_a == q.grid_a &&
              p.hess_first == q.hess_first && p.close_first == q.close_first && p.becomes == q.becomes &&
              p.joins_fix_list == q.joins_fix_list && p.backsolved == q.backsolved && p.nl == q.nl;
  for (int i = 0; same && i < p.nl; ++i) {
    const ss_launch &a = p.l[i], &b = q.l[i];
    same = a.op == b.op && (a.grid == b.grid || a.op == SS_SWEEP_B) && a.mode == b.mode && a.host_wgs == b.host_wgs && a.who == b.who &&
           a.wk == b.wk && a.wsb == b.wsb && a.nostore == b.nostore && a.raw_last == b.raw_last;
  }
  return same;
}
// NK_SS_RO and NK_SS_RO_GRID choose sweep B's grid and nothing else: the cycle planned without them, block by block
static void check_grid_b_only(tally &t, const ss_cycle_cfg &c, const ss_switches &sw) {
  for (int v = 0; v < 3; ++v) {
    ss_switches sx = sw;
    sx.ro = v & 1; sx.ro_grid = v & 2;
    ss_cycle_state st = ss_plan_begin(c), sy = ss_plan_begin(c);
    while (ss_plan_more(c, st) && ss_plan_more(c, sy)) {
      const ss_block_plan p = ss_plan_block(c, sw, st), q = ss_plan_block(c, sx, sy);
      if (!same_but_grid_b(p, q)) violation(t, "NK_SS_RO / NK_SS_RO_GRID change more than sweep B's grid", c, sw, p);
      ss_cycle_state fa = st, fb = sy;
      if (!same_but_grid_b(ss_plan_finish(c, sw, fa), ss_plan_finish(c, sx, fb)))
        violation(t, "NK_SS_RO / NK_SS_RO_GRID change more than sweep B's grid", c, sw, p);
    }
    if (ss_plan_more(c, st) != ss_plan_more(c, sy)) violation(t, "NK_SS_RO / NK_SS_RO_GRID change the block list", c, sw, ss_block_plan{});
  }
}
// one cycle; after every block also what would close the cycle if the host stopped there
static void check_cycle(tally &t, const ss_cycle_cfg &c, const ss_switches &sw) {
  ss_cycle_state st = ss_plan_begin(c);
  int width_sum = 0;
  ++t.cycles;
  while (ss_plan_more(c, st)) {
    const bool raw_before = st.raw_on;
    const ss_block_plan p = ss_plan_block(c, sw, st);
    ++t.blocks;
    width_sum += p.sb;
    if (p.sb < 1 || st.k != 1 + width_sum || st.k - 1 > c.steps) violation(t, "widths do not add up", c, sw, p);
    if (p.blk >= c.nblk_slots || st.blk != p.blk + 1) violation(t, "more blocks than factor slots", c, sw, p);
    if (st.nfix > c.nfix) violation(t, "fix list overflows", c, sw, p);
    if (p.host_a && !(c.single_rank && c.fixed_work)) violation(t, "host_a off one rank or fixed work", c, sw, p);
    if (raw_before) violation(t, "a block behind the unstored one", c, sw, p);
    check_launches(t, c, sw, p, raw_before);
    ss_cycle_state stop = st;
    const ss_block_plan f = ss_plan_finish(c, sw, stop);
    check_launches(t, c, sw, f, st.raw_on);
    if (stop.dp.on || stop.pend.sb > 0) violation(t, "something pending after the finish", c, sw, p);
    if (p.raw_last) {
      const ss_launch *last = f.nl > 0 ? &f.l[f.nl - 1] : nullptr;
      if (ss_plan_more(c, st) || !last || last->op != SS_JOB || !(last->mode & SSJ_BACK) || !last->raw_last || !f.backsolved)
        violation(t, "unstored block without a closing back-substitution", c, sw, p);
    }
  }
  if (width_sum != c.steps) violation(t, "widths do not add up to the steps", c, sw, ss_block_plan{});
}

static long long arg(int argc, char **argv, const char *key, long long dflt) {
  const size_t n = std::strlen(key);
  for (int i = 2; i < argc; ++i)
    if (std::strncmp(argv[i], key, n) == 0 && argv[i][n] == '=') return std::atoll(argv[i] + n + 1);
  return dflt;
}
int main(int argc, char **argv) {
  const std::string cmd = argc > 1 ? argv[1] : "";
  ss_cycle_cfg c;
  c.steps = (int)arg(argc, argv, "steps", 30);
  c.s = (int)arg(argc, argv, "s", 15);
  c.n = arg(argc, argv, "n", 1024 * 1024);
  c.ldv = arg(argc, argv, "ldv", c.n);
  c.v_aligned16 = arg(argc, argv, "aligned", 1) != 0;
  c.num_cus = (int)arg(argc, argv, "cus", 256);
  g_occ = (int)arg(argc, argv, "occ", 2);
  c.occupancy = occupancy;
  c.single_rank = arg(argc, argv, "single", 1) != 0;
  c.peer_ok = c.single_rank || arg(argc, argv, "peers", 1) != 0;
  c.newton = arg(argc, argv, "newton", 1) != 0;
  c.fixed_work = arg(argc, argv, "fixed", 1) != 0;
  c.auto_grow = arg(argc, argv, "grow", 0) != 0;
  c.accepts_back = arg(argc, argv, "back", 1) != 0;
  c.audit_on = arg(argc, argv, "audit", 0) != 0;
  const int slots = (int)arg(argc, argv, "slots", -1);   // slots=0: as many as steps, the most blocks a cycle can have
  c.nblk_slots = slots > 0 ? slots : c.steps + (slots < 0 ? 2 : 0);   // (the workspace: m + 2 with m ≥ steps)
  c.nfix = (int)arg(argc, argv, "nfix", 3);
  if (cmd == "cycle") {
    const ss_switches sw = ss_switches_from_env();
    const int stop_after = (int)arg(argc, argv, "stop", -1);
    ss_cycle_state st = ss_plan_begin(c);
    for (int b = 0; ss_plan_more(c, st) && b != stop_after; ++b) {
      const ss_block_plan p = ss_plan_block(c, sw, st);
      print_plan("block", p, st);
    }
    const ss_block_plan f = ss_plan_finish(c, sw, st);
    print_plan("finish", f, st);
    return 0;
  }
  if (cmd == "sweep") {
    // steps lo..hi × s 1..15 × growth × {one rank, peers, no peers} × basis × protocol × back-substitution accepted or not
    // × every on/off combination of the switches the planner reads (NK_SS_DEFER_HESS: unset, 0, 1)
    // flips=f: only the switch settings with at most f switches off their defaults — except at the steps listed in full_at=a,b,…
    // (the (steps, s) pairs are dealt out to as many threads as the machine has processors, at most 16)
    const int lo = (int)arg(argc, argv, "steps_lo", 1), hi = (int)arg(argc, argv, "steps_hi", 60);
    const int flips = (int)arg(argc, argv, "flips", 99), hold = (int)arg(argc, argv, "hold", 0);
    const bool grids = arg(argc, argv, "grids", 0) != 0;
    std::vector<bool> full(hi + 1, false);
    for (int i = 2; i < argc; ++i)
      if (std::strncmp(argv[i], "full_at=", 8) == 0)
        for (const char *q = argv[i] + 8; *q; q += std::strspn(q, ",")) {
          const int v = std::atoi(q);
          if (v >= lo && v <= hi) full[v] = true;
          q += std::strcspn(q, ",");
        }
    const int defaults = 0x1fff & ~128;   // (every on/off switch is on by default but NK_SS_LAST_SWEEP)
    unsigned nthr = std::thread::hardware_concurrency();
    nthr = nthr < 1 ? 1 : (nthr > 16 ? 16 : nthr);
    std::vector<tally> tallies(nthr);
    std::vector<std::thread> pool;
    for (unsigned ti = 0; ti < nthr; ++ti)
      pool.emplace_back([&, ti, c]() mutable {
        tally &t = tallies[ti];
        for (int item = (hi - lo + 1) * 15 - 1 - (int)ti; item >= 0; item -= (int)nthr) {   // (long cycles first)
          c.steps = lo + item / 15;
          c.s = 1 + item % 15;
          const int max_flips = full[c.steps] ? 99 : flips;
          for (int cf = 0; cf < 2 * 3 * 2 * 2 * 2; ++cf) {
            int q = cf;
            c.auto_grow = q % 2; q /= 2;
            c.single_rank = q % 3 == 0; c.peer_ok = q % 3 != 2; q /= 3;
            c.newton = q % 2; q /= 2;
            c.fixed_work = q % 2; q /= 2;
            c.accepts_back = q % 2;
            if (slots <= 0) c.nblk_slots = c.steps + (slots < 0 ? 2 : 0);
            for (int bits = 0; bits < (1 << 13); ++bits)
              for (int dh = -1; dh <= 1; ++dh) {
                if (__builtin_popcount(bits ^ defaults) + (dh != -1) > max_flips || ((bits ^ defaults) & hold)) continue;
                ss_switches sw;
                sw.fused = bits & 1; sw.grid_a = bits & 2; sw.kconst = bits & 4; sw.ro = bits & 8; sw.ro_grid = bits & 16;
                sw.mm = bits & 32; sw.implicit = bits & 64; sw.last_sweep = bits & 128; sw.host_a = bits & 256;
                sw.host_b = bits & 512; sw.defer = bits & 1024; sw.tail_back = bits & 2048; sw.nostore = bits & 4096;
                sw.defer_hess = dh;
                check_cycle(t, c, sw);
                if (grids && sw.ro && sw.ro_grid) check_grid_b_only(t, c, sw);
              }
          }
        }
      });
    tally t;
    for (unsigned ti = 0; ti < nthr; ++ti) {
      pool[ti].join();
      t.cycles += tallies[ti].cycles; t.blocks += tallies[ti].blocks; t.violations += tallies[ti].violations;
    }
    std::printf("{\"cycles\":%lld,\"blocks\":%lld,\"violations\":%lld}\n", t.cycles, t.blocks, t.violations);
    return t.violations ? 1 : 0;
  }
  std::fprintf(stderr, "usage: ss_plan_dump cycle|sweep [key=value …]\n");
  return 2;
}
