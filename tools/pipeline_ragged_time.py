"""Ragged blocks end to end, timing probe (development aid).

    pipeline_ragged_time.py [--repeats R] [--warmup W] [--out FILE]

Cities on the host to the final cost, log and merged tour on the host, wall
clock, two ways per shape in one process, the two alternating, R times after W
warm-up rounds; medians with min-max and every repeat are reported.

  uniform shapes   every block 16 cities (`./tsp 16 B 1000 1000`), 1024 and
                   16384 blocks at P = 1:
                     (u) tspgpu_pipeline_cities
                     (r) tspgpu_pipeline_cities_ragged with n = [16]*B
                   the expectation is parity; the ratio (r)/(u) is reported
  ragged shapes    n uniform in 8..16 (block b: the first n[b] cities of the
                   generator's 16-city block b), 16384 blocks at P = 1 and 8:
                     (c) the composition without the device hand-off:
                         solve_cities_ragged (costs, tours, statuses come
                         back), a numpy gather of the block paths,
                         tspgpu_reduce_ragged (host scans, upload)
                     (r) tspgpu_pipeline_cities_ragged

Cost, log and tour of the two ways are compared before anything is timed.  A
last line of JSON.  profiles/pipeline_ragged/ holds this report (--out)."""
import argparse, ctypes, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tsp-mpi-reduction_amd"), ROOT]
import numpy as np
import tspgpu
from bench import Shard  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default=None, help="also write the report to this file")
ap.add_argument("--uniform", default="1024x1,16384x1", help="B x P of the all-16 shapes, comma separated")
ap.add_argument("--ragged", default="16384x1,16384x8", help="B x P of the 8..16 shapes, comma separated")
args = ap.parse_args()

lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


ctx = tspgpu.Context(device=0)
L_ = tspgpu.lib()
cu, name = ctx.device_info()
say(f"device: {name}; repeats={args.repeats} warmup={args.warmup}")
cp = ctypes.POINTER(tspgpu.City)


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


def measure(case, paths, base):
    """paths: label -> fn, alternating; base: the label the others are a ratio of"""
    for _ in range(args.warmup):
        for fn in paths.values():
            fn()
    t = {k: [] for k in paths}
    for _ in range(args.repeats):
        for k, fn in paths.items():  # alternating
            t[k].append(wall(fn))
    res = {k: summary(v) for k, v in t.items()}
    for k in paths:
        show(case, k, res[k])
    a = res[base]["median_ms"]
    for k in paths:
        if k != base:
            res[k]["ratio_to_base"] = res[k]["median_ms"] / a
            say(f"{case} {k}: {res[k]['ratio_to_base']:.3f} x {base}'s wall time ({res[k]['median_ms'] - a:+.3f} ms)")
    return res


def same(a, b):
    """every component of two answers equal; says which one is not"""
    bad = [k for k, (x, y) in zip(("cost", "log", "ids", "x", "y"), zip(a, b)) if x != y]
    if bad:
        say(f"MISMATCH in {bad}: cost {a[0]!r} / {b[0]!r}, tour bytes {len(a[2])} / {len(b[2])}")
    return not bad


class Outputs:
    def __init__(self, cap):
        self.log = ctypes.create_string_buffer(1 << 20)
        self.final, self.plen = ctypes.c_double(), ctypes.c_int()
        self.cap = cap
        self.out = np.zeros(cap, dtype=tspgpu.CITY_DTYPE)

    def answer(self):
        tour = self.out[:self.plen.value]  # (field by field: the struct's padding bytes are nobody's)
        return (self.final.value, self.log.value, tour["id"].tobytes(), tour["x"].tobytes(), tour["y"].tobytes())


def run_uniform(B, P):
    n = 16
    case = f"16x{B} P={P}"
    sh = Shard(n, B, 0, B)
    ns = np.full(B, n, dtype=np.int32)
    o = Outputs(6 * B * (n + 1))

    def uniform():
        rc = L_.tspgpu_pipeline_cities(ctx.handle, sh.arr, n, B, P, ctypes.byref(o.final), o.out.ctypes.data_as(cp),
                                       o.cap, ctypes.byref(o.plen), o.log, len(o.log))
        assert rc == 0, rc
        return o.answer()

    def ragged():
        rc = L_.tspgpu_pipeline_cities_ragged(ctx.handle, sh.arr, tspgpu._ip(ns), B, P, ctypes.byref(o.final),
                                              o.out.ctypes.data_as(cp), o.cap, ctypes.byref(o.plen), o.log,
                                              len(o.log))
        assert rc == 0, rc
        return o.answer()

    assert same(uniform(), ragged())  # the same answer, before any clock
    return measure(case, {"(u) pipeline_cities": uniform, "(r) pipeline_cities_ragged": ragged},
                   "(u) pipeline_cities")


def run_ragged(B, P):
    case = f"8..16x{B} P={P}"
    rng = np.random.default_rng(816 + B + P)
    ns = rng.integers(8, 17, size=B).astype(np.int32)
    full = np.frombuffer(Shard(16, B, 0, B).arr, dtype=tspgpu.CITY_DTYPE, count=B * 16).reshape(B, 16)
    cities = np.ascontiguousarray(np.concatenate([full[b, :ns[b]] for b in range(B)]))
    arr = (tspgpu.City * len(cities)).from_buffer_copy(cities.tobytes())
    Ls = ns + 1
    city0 = np.concatenate(([0], np.cumsum(ns)[:-1])).astype(np.int64)
    total = int(Ls.sum())
    # the numpy gather: path city k of block b is cities[city0[b] + tour[b, k]]
    blk = np.repeat(np.arange(B), Ls)
    col = np.arange(total) - np.repeat(np.concatenate(([0], np.cumsum(Ls)[:-1])), Ls)
    stride = int(ns.max()) + 1
    lens = Ls.astype(np.int32)
    o = Outputs(6 * total)

    def composition():
        cost, tour, status = ctx.solve_cities_ragged((arr, ns), tour_stride=stride)
        assert not status.any()
        paths = np.ascontiguousarray(cities[city0[blk] + tour[blk, col]])
        rc = L_.tspgpu_reduce_ragged(ctx.handle, paths.ctypes.data_as(cp), tspgpu._ip(lens), tspgpu._dp(cost), B, P,
                                     ctypes.byref(o.final), o.out.ctypes.data_as(cp), o.cap, ctypes.byref(o.plen),
                                     o.log, len(o.log))
        assert rc == 0, rc
        return o.answer()

    def ragged():
        rc = L_.tspgpu_pipeline_cities_ragged(ctx.handle, arr, tspgpu._ip(ns), B, P, ctypes.byref(o.final),
                                              o.out.ctypes.data_as(cp), o.cap, ctypes.byref(o.plen), o.log,
                                              len(o.log))
        assert rc == 0, rc
        return o.answer()

    assert same(composition(), ragged())  # the same answer, before any clock
    res = measure(case, {"(c) solve + numpy gather + reduce": composition, "(r) pipeline_cities_ragged": ragged},
                  "(c) solve + numpy gather + reduce")
    say(f"{case} blocks per size: " + " ".join(f"{k}:{int((ns == k).sum())}" for k in range(8, 17)) +
        f"; merged tour {o.plen.value} cities")
    return res


result = {"device": name, "repeats": args.repeats}
for shape in filter(None, args.uniform.split(",")):
    B, P = map(int, shape.split("x"))
    result[f"16x{shape}"] = run_uniform(B, P)
for shape in filter(None, args.ragged.split(",")):
    B, P = map(int, shape.split("x"))
    result[f"8..16x{shape}"] = run_ragged(B, P)
say(json.dumps(result))
ctx.close()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
