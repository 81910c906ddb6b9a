"""Developer tool: the bench step with / without the C2PSA cv1 -> qkv pointwise chain, each on the register-weight executor
(chain_fast=1, block_chain_kernel) and on block_tile_kernel (chain_fast=0), alternating.  python tools/chain_ab.py [--rounds N] [bench options]"""
import json, os, subprocess, sys
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
code = ("import sys; sys.path.insert(0, %r); from edge_yolo_amd.nn.modules import block; block._Chains.pw_chains = %s; import bench; "
        "bench.main(['--steps', '200', '--warmup', '20', '--no-api', '--no-cpu-baseline', '--no-roofline', '--tune', 'chain_fast=%d'] + sys.argv[1:])")
args = sys.argv[1:]
rounds = 3
if "--rounds" in args:
    i = args.index("--rounds")
    rounds = int(args[i + 1])
    del args[i:i + 2]
forms = [("('proj_ffn_cv2',)", 0), ("('proj_ffn_cv2',)", 1), ("('proj_ffn_cv2', 'cv1_qkv')", 0), ("('proj_ffn_cv2', 'cv1_qkv')", 1)]
times = {}
for rnd in range(rounds):
    for chains, fast in forms:
        for extra in ([], ["--no-pipeline"]):
            r = subprocess.run([sys.executable, "-c", code % (root, chains, fast)] + args + extra, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:  # (a fault or an abort: nothing more is started on the GPU)
                sys.exit(f"bench exited with {r.returncode}:\n{r.stderr[-2000:]}")
            line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
            mode = "single-graph" if extra else "pipelined"
            ms = json.loads(line)["ms_per_step"]
            times.setdefault((mode, chains, fast), []).append(ms)
            print(f"  run {rnd + 1} {mode} pw_chains={chains} chain_fast={fast}: {ms:.4f} ms/step", flush=True)
for (mode, chains, fast), v in sorted(times.items()):
    s = sorted(v)
    print(f"  {mode} pw_chains={chains} chain_fast={fast}: {' '.join(f'{x:.4f}' for x in v)} | median {s[len(s) // 2]:.4f} min {s[0]:.4f} max {s[-1]:.4f}")
