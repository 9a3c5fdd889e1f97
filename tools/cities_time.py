"""Device distance build timing probe (development aid).

    cities_time.py [--blocks B] [--small S] [--repeats R] [--warmup W]

End to end from host cities of the reference generator (`./tsp 16 B 1000 1000`)
to costs and tours on the host, wall clock, for B blocks (default 65536) and a
small batch (default 512), 16 cities each:

  host      Context.solve_cities: tspgpu_distance_matrix on the host (glibc
            pow twice per entry), the matrices uploaded, K1
  upload    Context.solve_cities(device_dist=True): the cities uploaded, the
            matrices built on the device (the host's pow on the flagged
            squares only), the ragged path, K1
  resident  solve_cities_device on cities already in device memory, up to the
            end of the solve (no download)

The three run interleaved, R times after W warm-up rounds; median, min and max
are reported.  Then the phases of the device path, each its own measurement:
the build up to the end of its synchronisation (kernel A + the copy of the
list) and the host's pow (tspgpu_cities_last_phase_ms, host clock), the whole
tspgpu_distance_matrix_device (HIP events, so patch + finish + the copy back
of the results = whole - build - pow), the ragged solve on the resident
matrices and the plain K1 on them (HIP events), and the host's
tspgpu_distance_matrix alone.  The answers of the paths are compared bit for
bit before anything is timed.  A last line of JSON."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tsp-mpi-reduction_amd"), ROOT]
import numpy as np
import tspgpu
from bench import Shard  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--blocks", type=int, default=65536)
ap.add_argument("--small", type=int, default=512)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
args = ap.parse_args()
n = 16

ctx = tspgpu.Context(device=0)
cu, name = ctx.device_info()
print(f"device: {name}; n={n} repeats={args.repeats} warmup={args.warmup}", flush=True)


def summary(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)),
            "repeats_ms": [round(float(x), 3) for x in ms]}


def show(case, label, s):
    print(f"{case} {label:<34} median={s['median_ms']:9.3f} ms min={s['min_ms']:9.3f} max={s['max_ms']:9.3f} "
          f"({' '.join(f'{x:.2f}' for x in s['repeats_ms'])})", flush=True)


def wall(fn):
    t0 = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t0)


def events(fn):
    ctx.timer_start()
    fn()
    return ctx.timer_stop()


def run(B):
    case = f"B={B}"
    sh = Shard(n, B, 0, B)
    cities = (sh.arr, n, B)
    d_c = ctx.upload(np.frombuffer(sh.arr, dtype=np.uint8))
    d_d = ctx.alloc(B * n * n * 8)
    d_cost, d_tour, d_st = ctx.alloc(B * 8), ctx.alloc(B * (n + 1) * 4), ctx.alloc(B * 4)
    d_cost2, d_tour2 = ctx.alloc(B * 8), ctx.upload(np.full((B, n + 1), -1, dtype=np.int32))
    off = np.arange(B, dtype=np.int64) * (n * n)
    ns = np.full(B, n, dtype=np.int32)

    def host():
        return ctx.solve_cities(cities)

    def upload():
        return ctx.solve_cities(cities, device_dist=True)

    def resident():
        ctx.solve_cities_device(d_c, n, B, d_cost, d_tour, d_st, ctx.stream)
        ctx.synchronize()

    def build():
        ctx.distance_matrix_device(d_c, n, B, d_d, ctx.stream)

    def ragged():
        ctx.solve_ragged_device(d_d, tspgpu.F64, off, ns, d_cost, d_tour, n + 1, d_st, ctx.stream)

    def k1():
        ctx.solve_device(d_d, n, B, d_cost2, d_tour2, ctx.stream)

    # the same bits on every path, before any clock
    (c_h, t_h), (c_u, t_u) = host(), upload()
    resident()
    assert np.array_equal(c_h.view(np.uint64), c_u.view(np.uint64)) and np.array_equal(t_h, t_u)
    assert np.array_equal(c_h.view(np.uint64), ctx.download(d_cost, (B,), np.uint64))
    assert np.array_equal(t_h, ctx.download(d_tour, (B, n + 1), np.int32))
    assert not ctx.download(d_st, (B,), np.int32).any()
    build()
    ctx.synchronize()
    assert np.array_equal(sh.distances().view(np.uint64), ctx.download(d_d, (B, n, n), np.uint64))
    sq, flagged, passes = ctx.cities_last_fixups()

    paths = {"host (solve_cities)": host, "upload (device_dist=True)": upload, "resident (solve_cities_device)": resident}
    for _ in range(args.warmup):
        for fn in paths.values():
            fn()
    t = {k: [] for k in paths}
    for _ in range(args.repeats):
        for k, fn in paths.items():  # interleaved
            t[k].append(wall(fn))
    out = {k: summary(v) for k, v in t.items()}
    for k in paths:
        show(case, k, out[k])
    base = out["host (solve_cities)"]["median_ms"]
    for k in list(paths)[1:]:
        out[k]["ratio_to_host"] = out[k]["median_ms"] / base
        print(f"{case} {k}: {out[k]['ratio_to_host']:.3f} x the host path's wall time", flush=True)

    # phases, interleaved as well
    ph = {k: [] for k in ("build: kernel A + list copy + sync (host clock)", "host pow on the flagged (host clock)",
                          "distance_matrix_device whole (events)", "patch + finish + results up (difference)",
                          "ragged solve on resident matrices (events)", "plain K1 on resident matrices (events)",
                          "tspgpu_distance_matrix on the host (host clock)")}
    keys = list(ph)
    for r in range(args.warmup + args.repeats):
        whole = events(build)
        b_ms, p_ms = ctx.cities_last_phase_ms()
        rg = events(ragged)
        kk = events(k1)
        hd = wall(sh.distances)
        if r >= args.warmup:
            for k, v in zip(keys, (b_ms, p_ms, whole, whole - b_ms - p_ms, rg, kk, hd)):
                ph[k].append(v)
    out["phases"] = {k: summary(v) for k, v in ph.items()}
    for k in keys:
        show(case, k, out["phases"][k])
    out["squares"], out["flagged"], out["build_passes"] = sq, flagged, passes
    print(f"{case} squares={sq} flagged={flagged} ({100.0 * flagged / max(1, sq):.2f}%) build passes={passes}; "
          f"bytes: cities up {B * n * 24 / 1e6:.1f} MB, list down {8 * (sq // 4) / 1e6:.1f} MB (the list's capacity), "
          f"results up {8 * flagged / 1e6:.1f} MB; the host path uploads {B * n * n * 8 / 1e6:.1f} MB", flush=True)
    for p in (d_c, d_d, d_cost, d_tour, d_st, d_cost2, d_tour2):
        ctx.free(p)
    return out


result = {"device": name, "n": n, "repeats": args.repeats}
for B in (args.blocks, args.small):
    result[str(B)] = run(B)
print(json.dumps(result))
ctx.close()
