"""Wall time of learn_kmeans(device='cuda') at the shipped geometry (262 144 x 768 features, K = 1024, the reference's default keywords
n_init=20, max_iter=100, batch_size=10000), split into seeding / mini-batch loop / final inertia with HIP events: one warm-up, three
timed runs, median and spread.  With --host, sklearn's fit (device=None) once on the machine's CPUs for comparison.

    python tools/kmeans_fit_probe.py [--rows 262144] [--dim 768] [--clusters 1024] [--runs 3] [--host] [--out FILE.json]

The features are a planted mixture (tests/kmeans_fit_ref.planted_mixture); the loop stops where max_no_improvement=100 fires."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=262144)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--clusters", type=int, default=1024)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--host", action="store_true", help="also time sklearn's fit (device=None) once")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures the GPU fit: it needs an MI355X"
    import kmeans_fit_ref as R
    from open_musiclm_amd.kmeans_fit import GpuMiniBatchKMeans
    X = R.planted_mixture(a.rows, a.dim, a.clusters, scale=3.0, seed=0)
    x = torch.from_numpy(X).cuda()
    runs = []
    for i in range(a.runs + 1):
        km = GpuMiniBatchKMeans(n_clusters=a.clusters, seed=i, device="cuda")           # the reference's default keywords
        km.record_times = True
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        km.fit(x)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        rec = {"seeding": km.times_ms_["seeding"], "loop": km.times_ms_["loop"], "final_inertia": km.times_ms_["inertia"], "wall": wall,
               "n_steps": km.n_steps_, "stop": km.stop_reason_, "inertia_value": km.inertia_}
        print(("warm-up " if i == 0 else f"run {i}   ") + json.dumps(rec), flush=True)
        if i:
            runs.append(rec)
    res = {"rows": a.rows, "dim": a.dim, "clusters": a.clusters, "runs": runs}
    for key in ("seeding", "loop", "final_inertia", "wall"):
        v = [r[key] for r in runs]
        res[key + "_ms"] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
    if a.host:
        try:
            import sklearn  # noqa: F401
            from open_musiclm_amd.hf_hubert_kmeans import learn_kmeans
            import threading
            done = threading.Event()

            def heartbeat():                      # a silent fit of minutes looks like a hang to a job runner
                while not done.wait(60.0):
                    print(f"host fit running, {time.perf_counter() - t0:.0f} s", flush=True)
            with tempfile.TemporaryDirectory() as d:
                t0 = time.perf_counter()
                threading.Thread(target=heartbeat, daemon=True).start()
                km = learn_kmeans(X, 1, os.path.join(d, "km.joblib"), n_clusters=a.clusters, verbose=0)
                res["host_sklearn_s"] = time.perf_counter() - t0
                done.set()
                res["host_sklearn_inertia"] = float(-km.score(X) / len(X))
                res["host_cpus"] = int(os.environ.get("OMP_NUM_THREADS", 0)) or os.cpu_count()
        except ImportError:
            res["host_sklearn_s"] = None
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
