"""Or-opt stage timing and gain probe (development aid).

    or_opt_time.py [--repeats R] [--warmup W] [--max-passes P] [--shapes ..] [--segs ..] [--out FILE] [--append]

For the reference generator's batches 16 x 16384 and 8 x 1024 (`./tsp n B 1000
1000`, one rank), the two tours of tools/two_opt_time.py and its method: the
merged tour of tspgpu_pipeline_cities, tspgpu_two_opt_path on it (ring 2, run
to its stop), then tspgpu_or_opt_path on that result with ring 2 and max_seg
1, 2 and 3, run to its stop.  Reported per shape, and per (shape, max_seg):

  the 2-opt run's passes, wall time and search time per pass, from the same
  process, to set the Or-opt search beside;
  passes to the stop, candidates sent to the selection, moves applied;
  tspgpu_path_length after 2-opt, after 2-opt + Or-opt, and after each of the
  two followed by tspgpu_refine_path(m = 15); 2-opt + Or-opt + refinement must
  be strictly shorter than 2-opt + refinement: the run asserts it;
  wall time of the Or-opt call (host form: the tour goes up and comes back),
  median of R runs after W warm-ups, and per pass;
  the library's phase times: grid (bounds + grid build, once), search and
  apply (HIP events, summed over the passes), select (host clock), and what
  is left of the wall time: the per-pass copies and synchronisations.

The stage is deterministic: every repeat must return the same tour, and the
run checks it.  A last line of JSON per invocation.
profiles/or_opt/or_opt_time.txt is this report (--out; --append adds one
shape's run to the file of another's)."""
import argparse, ctypes, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tsp-mpi-reduction_amd"), ROOT]
import numpy as np
import tspgpu
from bench import Shard  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--max-passes", type=int, default=100000)
ap.add_argument("--interior", type=int, default=15, help="m of the refinement the stages are composed with")
ap.add_argument("--ring", type=int, default=2)
ap.add_argument("--out", default=None, help="also write the report to this file")
ap.add_argument("--append", action="store_true", help="add to --out instead of replacing it")
ap.add_argument("--shapes", default="16x16384,8x1024", help="n x B, comma separated")
ap.add_argument("--segs", default="1,2,3")
args = ap.parse_args()

lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


ctx = tspgpu.Context(device=0)
L_ = tspgpu.lib()
cu, name = ctx.device_info()
cp = ctypes.POINTER(tspgpu.City)
say(f"device: {name}; repeats={args.repeats} warmup={args.warmup} max_passes={args.max_passes} ring={args.ring} "
    f"refine m={args.interior}")


def wall(fn):
    t0 = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t0)


def length(arr, L):
    out = ctypes.c_double()
    assert L_.tspgpu_path_length(arr.ctypes.data_as(cp), L, ctypes.byref(out)) == 0
    return out.value


def refined(src, L):
    out = np.zeros(L, dtype=tspgpu.CITY_DTYPE)
    st = tspgpu.RefineStats()
    rc = L_.tspgpu_refine_path(ctx.handle, src.ctypes.data_as(cp), L, args.interior, 64, out.ctypes.data_as(cp),
                               ctypes.byref(st))
    assert rc == 0, rc
    return length(out, L)


def timed(call, out, st):
    """-> (stats dict, wall ms of each repeat, median phase ms) of a stage run
    `repeats` times after the warm-ups, every run giving the same tour."""
    for _ in range(args.warmup):
        call()
    call()
    first = out.view(np.uint8).copy()  # (raw bytes: a structured copy leaves the padding undefined)
    ms, ph = [], []
    for _ in range(args.repeats):
        ms.append(wall(call))
        ph.append((st.grid_ms, st.search_ms, st.select_ms, st.apply_ms))
        assert np.array_equal(out.view(np.uint8), first)  # deterministic
    return st.as_dict(), ms, tuple(float(np.median([e[i] for e in ph])) for i in range(4))


def run(n, B):
    case = f"{n}x{B}"
    sh = Shard(n, B, 0, B)
    cap = B * n + 1
    tour = np.zeros(cap, dtype=tspgpu.CITY_DTYPE)
    log = ctypes.create_string_buffer(1 << 20)
    final, plen = ctypes.c_double(), ctypes.c_int()
    rc = L_.tspgpu_pipeline_cities(ctx.handle, sh.arr, n, B, 1, ctypes.byref(final), tour.ctypes.data_as(cp), cap,
                                   ctypes.byref(plen), log, len(log))
    assert rc == 0, rc
    L = plen.value
    merged = length(tour, L)

    two = np.zeros(L, dtype=tspgpu.CITY_DTYPE)
    tst = tspgpu.TwoOptStats()

    def two_opt():
        rc = L_.tspgpu_two_opt_path(ctx.handle, tour.ctypes.data_as(cp), L, args.ring, args.max_passes,
                                    two.ctypes.data_as(cp), ctypes.byref(tst))
        assert rc == 0, rc

    ts, tms, (_, tsearch, tselect, _) = timed(two_opt, two, tst)
    before = length(two, L)
    two_refined = refined(two, L)
    tp = max(1, ts["passes"])
    res = {"tour_cities": L, "length_merged": merged, "length_two_opt": before, "length_two_opt_refine": two_refined,
           "two_opt": {"passes": ts["passes"], "moves": ts["moves"], "wall_ms": float(np.median(tms)),
                       "search_ms": tsearch, "search_ms_per_pass": tsearch / tp, "select_ms": tselect}}
    say(f"{case} tour {L} cities, path_length {merged:.6f}; 2-opt ring={args.ring}: {ts['passes']} passes, "
        f"{ts['moves']} moves -> {before:.6f}, wall median {np.median(tms):.3f} ms, search {tsearch:.3f} ms = "
        f"{tsearch / tp:.3f} ms/pass, select (host) {tselect:.3f} ms; after refine(m={args.interior}) {two_refined:.6f}")
    for seg in map(int, args.segs.split(",")):
        out = np.zeros(L, dtype=tspgpu.CITY_DTYPE)
        st = tspgpu.OrOptStats()

        def or_opt():
            rc = L_.tspgpu_or_opt_path(ctx.handle, two.ctypes.data_as(cp), L, args.ring, seg, args.max_passes,
                                       out.ctypes.data_as(cp), ctypes.byref(st))
            assert rc == 0, rc

        s, ms, (grid, search, select, apply_) = timed(or_opt, out, st)
        after = length(out, L)
        both = refined(out, L)
        assert np.array_equal(np.sort(out["id"]), np.sort(two["id"])) and out[0] == two[0] and out[L - 1] == two[L - 1]
        assert after < before, (after, before)
        assert both < two_refined, (both, two_refined)  # the one condition: the stages compose
        p = max(1, s["passes"])
        med = float(np.median(ms))
        rest = med - (grid + search + select + apply_)
        res[f"max_seg={seg}"] = {"passes": s["passes"], "candidates": s["candidates"], "moves": s["moves"],
                                 "gain": s["gain"], "length_after": after, "length_after_refine": both,
                                 "shorter_percent": 100.0 * (before - after) / before,
                                 "shorter_percent_with_refine": 100.0 * (two_refined - both) / two_refined,
                                 "wall_ms": {"median": med, "repeats": [round(x, 3) for x in ms]},
                                 "wall_ms_per_pass": med / p, "search_ms_per_pass": search / p,
                                 "phase_ms": {"grid": grid, "search": search, "select": select, "apply": apply_,
                                              "copies_and_syncs": rest},
                                 "stopped_by_rule": s["passes"] < args.max_passes}
        say(f"{case} max_seg={seg}: {s['passes']} passes{'' if s['passes'] < args.max_passes else ' (max_passes reached)'}, "
            f"{s['candidates']} candidates, {s['moves']} moves | path_length {before:.6f} -> {after:.6f} "
            f"({100.0 * (before - after) / before:.3f}% shorter; gain {s['gain']:.6f}) -> {both:.6f} after "
            f"refine(m={args.interior}) ({100.0 * (two_refined - both) / two_refined:.3f}% shorter than 2-opt + refine)")
        say(f"{case} max_seg={seg}: wall median {med:.3f} ms ({' '.join(f'{x:.2f}' for x in ms)}) = {med / p:.3f} ms/pass; "
            f"phase ms: grid {grid:.3f}, search {search:.3f} = {search / p:.3f} ms/pass, select (host) {select:.3f}, "
            f"apply {apply_:.3f}, copies + syncs {rest:.3f}")
    return res


result = {"device": name, "repeats": args.repeats, "max_passes": args.max_passes, "ring": args.ring,
          "refine_m": args.interior}
for shape in args.shapes.split(","):
    n, B = map(int, shape.split("x"))
    result[shape] = run(n, B)
say(json.dumps(result))
ctx.close()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as f:
        f.write("\n".join(lines) + "\n")
