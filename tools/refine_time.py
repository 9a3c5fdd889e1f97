"""Window refinement timing and gain probe (development aid).

    refine_time.py [--repeats R] [--warmup W] [--max-passes P] [--out FILE]

For the reference generator's batches 16 x 16384 and 8 x 1024 (`./tsp n B 1000
1000`, one rank): the merged tour of tspgpu_pipeline_cities, then
tspgpu_refine_path on it with m = 7, 12 and 15 interior cities per window,
run to its stop (max_passes is generous).  Reported per (shape, m):

  passes to the stop, windows solved / replaced / skipped;
  tspgpu_path_length before and after, and the library's gain;
  wall time of the refinement (host form: the tour goes up and comes back),
  median of R runs after W warm-ups, and per pass;
  device time per pass (HIP events inside the library) split into build
  (window gather + exact distance build, the host's pow included), K1 (with
  its validating gather and scatter) and fold + apply;
  the wall time of the pipeline_cities call that made the tour, measured in
  the same process, for scale.

The refinement is deterministic: every repeat must return the same tour, and
the run checks it.  A last line of JSON.  profiles/refine/refine_time.txt is
this report (--out)."""
import argparse, ctypes, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tsp-mpi-reduction_amd"), ROOT]
import numpy as np
import tspgpu
from bench import Shard  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--max-passes", type=int, default=64)
ap.add_argument("--out", default=None, help="also write the report to this file")
ap.add_argument("--shapes", default="16x16384,8x1024", help="n x B, comma separated")
ap.add_argument("--interiors", default="7,12,15")
args = ap.parse_args()

lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


ctx = tspgpu.Context(device=0)
L_ = tspgpu.lib()
cu, name = ctx.device_info()
cp = ctypes.POINTER(tspgpu.City)
say(f"device: {name}; repeats={args.repeats} warmup={args.warmup} max_passes={args.max_passes}")


def wall(fn):
    t0 = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t0)


def length(arr, L):
    out = ctypes.c_double()
    assert L_.tspgpu_path_length(arr.ctypes.data_as(cp), L, ctypes.byref(out)) == 0
    return out.value


def run(n, B):
    case = f"{n}x{B}"
    sh = Shard(n, B, 0, B)
    cap = B * n + 1
    tour = np.zeros(cap, dtype=tspgpu.CITY_DTYPE)
    log = ctypes.create_string_buffer(1 << 20)
    final, plen = ctypes.c_double(), ctypes.c_int()

    def pipeline():
        rc = L_.tspgpu_pipeline_cities(ctx.handle, sh.arr, n, B, 1, ctypes.byref(final), tour.ctypes.data_as(cp), cap,
                                       ctypes.byref(plen), log, len(log))
        assert rc == 0, rc

    for _ in range(args.warmup):
        pipeline()
    pipe_ms = [wall(pipeline) for _ in range(args.repeats)]
    L = plen.value
    before = length(tour, L)
    res = {"tour_cities": L, "pipeline_cities_ms": {"median": float(np.median(pipe_ms)),
                                                    "repeats": [round(x, 3) for x in pipe_ms]},
           "length_before": before, "pipeline_cost": final.value}
    say(f"{case} pipeline_cities: median {np.median(pipe_ms):.3f} ms ({' '.join(f'{x:.2f}' for x in pipe_ms)}); "
        f"tour {L} cities, path_length {before:.6f} (the reference's cost {final.value:.6f})")
    for m in map(int, args.interiors.split(",")):
        out = np.zeros(L, dtype=tspgpu.CITY_DTYPE)
        st = tspgpu.RefineStats()

        def refine():
            rc = L_.tspgpu_refine_path(ctx.handle, tour.ctypes.data_as(cp), L, m, args.max_passes,
                                       out.ctypes.data_as(cp), ctypes.byref(st))
            assert rc == 0, rc

        for _ in range(args.warmup):
            refine()
        first = out.view(np.uint8).copy()  # (raw bytes: a structured copy leaves the padding undefined)
        ms, ev = [], []
        for _ in range(args.repeats):
            ms.append(wall(refine))
            ev.append((st.build_ms, st.k1_ms, st.fold_apply_ms))
            assert np.array_equal(out.view(np.uint8), first)  # deterministic
        s = st.as_dict()
        after = length(out, L)
        assert np.array_equal(np.sort(out["id"]), np.sort(tour["id"][:L])) and out[0] == tour[0] and out[L - 1] == tour[L - 1]
        p = max(1, s["passes"])
        b, k, fa = (float(np.median([e[i] for e in ev])) for i in range(3))
        res[f"m={m}"] = {"passes": s["passes"], "windows": s["windows"], "replaced": s["replaced"],
                         "skipped": s["skipped"], "gain": s["gain"], "length_after": after,
                         "gain_percent": 100.0 * (before - after) / before,
                         "wall_ms": {"median": float(np.median(ms)), "repeats": [round(x, 3) for x in ms]},
                         "wall_ms_per_pass": float(np.median(ms)) / p,
                         "device_ms_per_pass": {"build": b / p, "k1": k / p, "fold_apply": fa / p},
                         "stopped_by_rule": s["passes"] < args.max_passes}
        say(f"{case} m={m:2d}: {s['passes']} passes{'' if s['passes'] < args.max_passes else ' (max_passes reached)'}, "
            f"{s['windows']} windows solved, {s['replaced']} replaced, {s['skipped']} skipped | path_length "
            f"{before:.6f} -> {after:.6f} ({100.0 * (before - after) / before:.3f}% shorter; gain {s['gain']:.6f})")
        say(f"{case} m={m:2d}: wall median {np.median(ms):.3f} ms ({' '.join(f'{x:.2f}' for x in ms)}) = "
            f"{np.median(ms) / p:.3f} ms/pass; device ms/pass: build {b / p:.3f}, K1 {k / p:.3f}, "
            f"fold+apply {fa / p:.3f}; {np.median(ms) / np.median(pipe_ms):.2f} x the pipeline_cities call")
    return res


result = {"device": name, "repeats": args.repeats, "max_passes": args.max_passes}
for shape in args.shapes.split(","):
    n, B = map(int, shape.split("x"))
    result[shape] = run(n, B)
say(json.dumps(result))
ctx.close()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
