"""K1-wide timing probe (development aid): single instances over the whole GPU.

    wide_time.py [--dtype f64|i32 ...] [--repeats R] [n ...]

--dtype f64 (default) times tspgpu_solve_instance on uniform Euclidean
distances, as before.  With i32 among the dtypes the matrix is the rounded
(TSPLIB nint) image of those distances and every dtype named runs on that
same matrix in this one process — `--dtype f64 i32` is the f64 / int32
comparison: per dtype the median, min and max of the entry's kernel_ms over
the repeats (after one untimed warm-up call), the table bytes, and the wall
time of the first call (allocation included)."""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tsp-mpi-reduction_amd"), ROOT]
import numpy as np
import tspgpu
from bench import Shard  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("n", nargs="*", type=int, default=[12, 16, 20, 24])
ap.add_argument("--dtype", nargs="+", choices=["f64", "i32"], default=["f64"])
ap.add_argument("--repeats", type=int, default=3)
args = ap.parse_args()

ctx = tspgpu.Context(device=0)
for n in args.n:
    rng = np.random.default_rng(n)
    xy = rng.uniform(0, 1000, size=(n, 2))
    d = tspgpu.distance_matrix([[(i, xy[i, 0], xy[i, 1]) for i in range(n)]])[0]
    if "i32" in args.dtype:
        d = np.rint(d)
    answers = []
    for dtype in args.dtype:
        solve = ctx.solve_instance_i32 if dtype == "i32" else ctx.solve_instance
        dd = d.astype(np.int32) if dtype == "i32" else d
        t = time.perf_counter()
        solve(dd)  # warm-up: code object load and the table's allocation
        first = (time.perf_counter() - t) * 1e3
        times = []
        for _ in range(args.repeats):
            t = time.perf_counter()
            cost, tour, ms = solve(dd)
            wall = (time.perf_counter() - t) * 1e3
            times.append(ms)
        answers.append((float(cost), tour.tolist()))
        table = (n - 1) * 2 ** (n - 2) * (4 if dtype == "i32" else 8)
        line = (f"n={n} dtype={dtype} cost={float(cost):.6f} wide kernel={min(times):.3f} ms "
                f"median={float(np.median(times)):.3f} max={max(times):.3f} (of {len(times)}) "
                f"table={table} B first_call_wall={first:.1f} ms wall={wall:.3f} ms")
        if n <= 20 and dtype == "f64":
            pd = ctx.upload(dd[None]); dc = ctx.alloc(8); dt = ctx.alloc((n + 1) * 4)
            ctx.solve_device(pd, n, 1, dc, dt, ctx.stream); ctx.synchronize()
            ctx.timer_start()
            for _ in range(5):
                ctx.solve_device(pd, n, 1, dc, dt, ctx.stream)
            k1 = ctx.timer_stop() / 5
            line += f"  K1 one-workgroup kernel={k1:.3f} ms"
        print(line, flush=True)
    assert all(a == answers[0] for a in answers), f"n={n}: the dtypes disagree: {answers}"
