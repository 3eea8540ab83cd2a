"""The prize of the warm role (lm_kernels.h WarmArgs), with nothing else running: the warm role
as a launch of its own (warm_probe_kernel: TTS_WARM_STAGES stages of a layer's gate/up stream
read into L2 by TTS_WARM_WGS workgroups, placed by TTS_WARM_XCD_DIST), then the product one-row
gate/up launch (TTS_GU_RING = 2 | 4), rotating over the layers so nothing is warm by accident.

The switches are read once per process, so one process measures one setting:
  as the program under the profiler (kernel times: HIP events are too coarse for 12-us launches)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python scripts/warm_probe.py run [ITERS]
  then, for every DIR/run_kernel_stats.csv written that way, one line per setting
    python scripts/warm_probe.py table LABEL=DIR [LABEL=DIR ...]"""
import csv
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(iters):
    sys.path.insert(0, os.path.join(ROOT, "tts-max_amd"))
    from tts_amd import configs
    from tts_amd.speechlm import MI355XSpeechLM

    m = MI355XSpeechLM.synthetic(configs.TTS1, max_batch=1, max_seq_len=1040)
    ms, _ = m.bench_kernel("warm_gate_up", rows=1, ctx=450, iters=iters)
    print(f"warm + gate/up, HIP events: {ms * 1e3:.2f} us per pair "
          f"(TTS_WARM_STAGES={os.environ.get('TTS_WARM_STAGES', '0')} TTS_GU_RING={os.environ.get('TTS_GU_RING', '2')} "
          f"TTS_WARM_WGS={os.environ.get('TTS_WARM_WGS', '120')} TTS_WARM_XCD_DIST={os.environ.get('TTS_WARM_XCD_DIST', '0')})")
    m.close()


def table(pairs):
    for pair in pairs:
        label, d = pair.split("=", 1)
        rows = list(csv.DictReader(open(os.path.join(d, "run_kernel_stats.csv"))))
        gu = [r for r in rows if "wgemm_kernel" in r["Name"] and "warm" not in r["Name"]]
        gu = max(gu, key=lambda r: int(r["Calls"]))  # (the timed launches; the set-up's run once)
        wm = [r for r in rows if "warm_probe_kernel" in r["Name"]]
        w = f"{float(wm[0]['AverageNs']) / 1e3:6.2f} us x {wm[0]['Calls']}" if wm else "   -"
        print(f"{label:28s} gate/up {float(gu['AverageNs']) / 1e3:6.2f} us avg (min {float(gu['MinNs']) / 1e3:6.2f}) x {gu['Calls']}   warm {w}")


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(int(sys.argv[2]) if len(sys.argv) > 2 else 320)
    else:
        table(sys.argv[2:])
