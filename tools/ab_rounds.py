"""The A/B protocol of profiles/r05_pair_base_ab.txt and r06_stream_policy_ab.txt: AB_ROUNDS (default 5) rounds of
`bench.py --gpus 1 --steps 100 --warmup 20 --no-cpu-baseline [AB_EXTRA]`, the libraries (BFCNN_HIP_LIB) alternating within a round in the
order given, every run a process of its own under its own time limit; stops at the first failure.  Prints images/s and the
HIP-event average of a block launch per run, then mean / min / max / min-max spread per library.
usage: python tools/ab_rounds.py OUT.txt lib1.so lib2.so ...      ("default" = the library the package loads by itself)"""
import json
import os
import subprocess
import sys

out_path, libs = sys.argv[1], sys.argv[2:]
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
rounds = int(os.environ.get("AB_ROUNDS", "5"))
extra = os.environ.get("AB_EXTRA", "").split()


def name(lib):
    return lib if lib == "default" else os.path.basename(lib).replace("libbfcnn_hip_", "").replace(".so", "")


os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
res = {lib: [] for lib in libs}
with open(out_path, "a") as log:
    def say(msg):
        print(msg, flush=True)
        log.write(msg + "\n")
        log.flush()

    for r in range(rounds):
        for lib in libs:
            env = dict(os.environ)
            if lib != "default":
                env["BFCNN_HIP_LIB"] = os.path.abspath(lib)
                if not os.path.exists(env["BFCNN_HIP_LIB"]):
                    sys.exit(f"no such library: {lib}")
            p = subprocess.run(["timeout", "-k", "10", "120", sys.executable, "bench.py", "--gpus", "1", "--steps", "100", "--warmup", "20",
                                "--no-cpu-baseline"] + extra, capture_output=True, text=True, env=env, cwd=root)
            line = [l for l in p.stdout.splitlines() if l.startswith("{")]
            if p.returncode != 0 or not line:
                say(f"round {r + 1} [{name(lib)}] FAILED rc={p.returncode}: {p.stderr[-600:]}")
                sys.exit(1)
            d = json.loads(line[-1])
            res[lib].append((d["value"], d["roofline"]["launch_us"]))
            say(f"round {r + 1} {name(lib):12s} {d['value']:9.1f} img/s  block launch {d['roofline']['launch_us']:7.2f} us")
    for lib in libs:
        v = [x[0] for x in res[lib]]
        say(f"{name(lib):12s} mean {sum(v) / len(v):9.1f}  min {min(v):9.1f}  max {max(v):9.1f}  spread {max(v) - min(v):6.1f}  "
            f"launch {sum(x[1] for x in res[lib]) / len(v):7.2f} us")
