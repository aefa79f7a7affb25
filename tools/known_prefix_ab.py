"""The known prefix on and off (switch skip_known) in ONE process, alternating, so that drift between processes cancels (as tools/sweep_items.py):

    python tools/known_prefix_ab.py [CONFIG] [MODE] [ROUNDS]

Per side and round 200 steps with the library's events off (ms per step), then 7 with all of them on: per pass the median of the whole pass
(gpu_ms), of its pair kernel alone (tile_ms) and their difference (the opener, the launch gaps), and from the last step's statistics
pairs_screened on both sides, pairs_known, and whether pairs_evaluated, new_keys and n_active_after agree.  pairs_screened - pairs_known is
what the pair kernel multiplied: the live items of a pass shrink with it (they are not counted on the device)."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch
    from tscode_amd.pipeline import DevicePipeline
    from tscode_amd.synthetic import make_config
    cfg = sys.argv[1] if len(sys.argv) > 1 else "C3"
    mode = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 4
    pipe = DevicePipeline(make_config(cfg), device_index=0, mode=mode)
    for _ in range(10):
        pipe.step()
    step_ms, pass_us, stats_of, ref = {1: [], 0: []}, {1: [], 0: []}, {}, None
    for rnd in range(rounds):
        for skip in (0, 1):
            pipe.set_option("skip_known", skip)
            pipe.set_option("pass_timing", 0)
            for _ in range(3):
                pipe.step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(200):
                r = pipe.step()
            torch.cuda.synchronize()
            step_ms[skip].append((time.perf_counter() - t0) / 200 * 1e3)
            pipe.set_option("pass_timing", 2)
            per, til = {}, {}
            for _ in range(7):
                r = pipe.step()
                torch.cuda.synchronize()
                for s in r["stats"]:
                    per.setdefault(int(s["k"]), []).append(s["gpu_ms"] * 1e3)
                    til.setdefault(int(s["k"]), []).append(s["tile_ms"] * 1e3)
            pass_us[skip].append({k: (statistics.median(v), statistics.median(til[k])) for k, v in per.items()})
            stats_of[skip] = r["stats"]
            if ref is None:
                ref = (r["n_pass"], r["n_keep"])
            assert (r["n_pass"], r["n_keep"]) == ref, (skip, r["n_pass"], r["n_keep"], ref)
    print(f"{cfg} mode {mode}: n_pass {ref[0]} n_keep {ref[1]}")
    for skip in (0, 1):
        print(f"skip_known {skip}: ms/step (events off) " + " ".join(f"{x:.4f}" for x in step_ms[skip]) + f"   median {statistics.median(step_ms[skip]):.4f}")
    print("pass k | pass us off | on | pair kernel us off | on | opener+rest us off | on | screened off | screened on | known | evaluated equal")
    for s0, s1 in zip(stats_of[0], stats_of[1]):
        k = int(s0["k"])
        a = [rd[k] for rd in pass_us[0]]; b = [rd[k] for rd in pass_us[1]]
        pa, pb = statistics.median(x[0] for x in a), statistics.median(x[0] for x in b)
        ta, tb = statistics.median(x[1] for x in a), statistics.median(x[1] for x in b)
        print(f"{k:5d} | {pa:6.1f} | {pb:6.1f} | {ta:6.1f} | {tb:6.1f} | {pa - ta:6.1f} | {pb - tb:6.1f} | {s0['pairs_screened']} | {s1['pairs_screened']} | {s1['pairs_known']} | "
              f"{s0['pairs_evaluated'] == s1['pairs_evaluated'] and s0['new_keys'] == s1['new_keys'] and s0['n_active_after'] == s1['n_active_after']} algo {s1['algo']}")


if __name__ == "__main__":
    main()
