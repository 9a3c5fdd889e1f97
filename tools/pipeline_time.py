"""K1 -> K3 hand-off timing probe (development aid).

    pipeline_time.py [--repeats R] [--warmup W] [--out FILE]

Cities of the reference generator (`./tsp n B 1000 1000`) on the host to the
final cost and log on the host, wall clock, two ways in one process:

  (a) host hand-off   solve_cities(device_dist=True): costs and tours come
                      back; the host gathers the block paths
                      (convPathToCityPath, here one numpy take); tspgpu_reduce
                      scans them three times and uploads them
  (b) device          tspgpu_pipeline_cities: K1's results stay on the GPU, the
                      gather / summary / uniqueness kernels, only the costs
                      visit the host; the merged tour comes back (one copy)
  (b0)                the same asked for no tour (path_cap 0), since (a)
                      returns none either

The three run interleaved, R times after W warm-up rounds, for 8 x 1024 at
P = 8, 16 x 1024 at P = 1 and 16 x 16384 at P = 1 and 8; medians and every
repeat are reported, and the device time of (b)'s gather, summary and
uniqueness kernels from HIP events (tspgpu_reduce_device_last_ms).  Cost and
log of the paths are compared before anything is timed.  A last line of
JSON.  profiles/pipeline/pipeline_time.txt is this report (--out)."""
import argparse, ctypes, errno, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tsp-mpi-reduction_amd"), ROOT]
import numpy as np
import tspgpu
from bench import Shard  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default=None, help="also write the report to this file")
ap.add_argument("--shapes", default="8x1024x8,16x1024x1,16x16384x1,16x16384x8", help="n x B x P, comma separated")
args = ap.parse_args()

lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


ctx = tspgpu.Context(device=0)
L_ = tspgpu.lib()
cu, name = ctx.device_info()
say(f"device: {name}; repeats={args.repeats} warmup={args.warmup}")


def summary(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)),
            "repeats_ms": [round(float(x), 3) for x in ms]}


def show(case, label, s):
    say(f"{case} {label:<34} median={s['median_ms']:9.3f} ms min={s['min_ms']:9.3f} max={s['max_ms']:9.3f} "
        f"({' '.join(f'{x:.2f}' for x in s['repeats_ms'])})")


def wall(fn):
    t0 = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t0)


def run(n, B, P):
    case = f"{n}x{B} P={P}"
    sh = Shard(n, B, 0, B)
    cities = np.frombuffer(sh.arr, dtype=tspgpu.CITY_DTYPE, count=B * n)
    L = tspgpu.tour_length(n)
    base = (np.arange(B, dtype=np.int64) * n)[:, None]
    log = ctypes.create_string_buffer(1 << 20)
    final, plen = ctypes.c_double(), ctypes.c_int()
    cap = (B * (L - 1) + 1) if P == 1 else 6 * B * L
    out = np.zeros(cap, dtype=tspgpu.CITY_DTYPE)
    cp = ctypes.POINTER(tspgpu.City)

    def host_handoff():
        cost, tour = ctx.solve_cities((sh.arr, n, B), device_dist=True)
        paths = np.ascontiguousarray(cities[(base + tour[:, :L]).ravel()])
        rc = L_.tspgpu_reduce(ctx.handle, paths.ctypes.data_as(cp), L, tspgpu._dp(cost), B, P, ctypes.byref(final),
                              log, len(log))
        assert rc == 0, rc
        return final.value, log.value

    def device(path_cap=cap):
        rc = L_.tspgpu_pipeline_cities(ctx.handle, sh.arr, n, B, P, ctypes.byref(final),
                                       out.ctypes.data_as(cp) if path_cap else None, path_cap, ctypes.byref(plen),
                                       log, len(log))
        assert rc == (0 if path_cap else -errno.ENOSPC), rc
        return final.value, log.value

    def device_no_tour():
        return device(0)

    # the same answer on every path, before any clock
    want = host_handoff()
    assert device() == want and device_no_tour() == want
    ids = out["id"][:plen.value]
    if P == 1:
        assert plen.value == B * n + 1 and ids[0] == ids[-1] and np.array_equal(np.sort(ids[:-1]), np.arange(B * n))

    paths = {"(a) host hand-off": host_handoff, "(b) device pipeline": device, "(b0) device, no tour": device_no_tour}
    for _ in range(args.warmup):
        for fn in paths.values():
            fn()
    t = {k: [] for k in paths}
    gather = []
    for _ in range(args.repeats):
        for k, fn in paths.items():  # interleaved
            t[k].append(wall(fn))
            if k.startswith("(b) "):
                gather.append(ctx.reduce_device_last_ms())
    res = {k: summary(v) for k, v in t.items()}
    for k in paths:
        show(case, k, res[k])
    res["gather + summary + uniqueness kernels (events)"] = summary(gather)
    show(case, "gather+summary+unique (events)", res["gather + summary + uniqueness kernels (events)"])
    a = res["(a) host hand-off"]["median_ms"]
    for k in list(paths)[1:]:
        res[k]["ratio_to_a"] = res[k]["median_ms"] / a
        say(f"{case} {k}: {res[k]['ratio_to_a']:.3f} x (a)'s wall time ({res[k]['median_ms'] - a:+.3f} ms)")
    say(f"{case} merged tour {plen.value} cities; bytes (a) moves and (b) does not: tours down "
        f"{B * (n + 1) * 4 / 1e6:.2f} MB, paths up {B * L * 24 / 1e6:.2f} MB; (b) brings the tour down: "
        f"{plen.value * 24 / 1e6:.2f} MB")
    return res


result = {"device": name, "repeats": args.repeats}
for shape in args.shapes.split(","):
    n, B, P = map(int, shape.split("x"))
    result[shape] = run(n, B, P)
say(json.dumps(result))
ctx.close()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
