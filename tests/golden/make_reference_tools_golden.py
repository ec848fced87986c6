"""Generates tests/golden/reference_tools_runs.json: what Granite's own tools/sweep_scene.py and tools/bench_aa.py do with our headless
runners.  Each script is executed against a stand-in binary that parses its command line with our argument parser, writes the --stat
document with headless.stat_document() and records both.  The file keeps, per script, the arguments it was started with, every
command line it built (temporary paths as {tmp} / {stat}), the stat document it read back after each call and the results document it
wrote.  tests/test_headless_tools_cpu.py checks our parsers and stat_document() against these records.

    python tests/golden/make_reference_tools_golden.py <Granite checkout>"""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# what each stand-in computes from its parsed command line; tests/test_headless_tools_cpu.py computes the same
SWEEP_STUB = """
from granite_amd import headless
args = headless.parse_args(sys.argv[1:])
kw = headless.viewer_config_to_kwargs(json.load(open(args.config)))
stamps = {"gbuffer-main + lighting-main": (7, 1.4), "tonemap": (7, 0.21)}
doc = headless.stat_document(250.0 if kw["post_aa"] == 0 else 300.0, "stub gpu", 42, stamps, args.frames)
"""
AA_STUB = """
from granite_amd import aa_bench, headless
args = aa_bench.parse_args(sys.argv[1:])
kw = aa_bench.method_to_kwargs(args.aa_method)
doc = headless.stat_document(100.0 + 10.0 * kw["post_aa"] + 20.0 * kw["pre_aa"], "stub gpu", 7, {"tonemap": (9, 0.9)}, args.frames)
"""
SWEEP_CONFIGS = {"plain": {"renderer": "deferred", "hdrBloom": True}, "fxaa": {"postAA": "fxaa"}}


def stub(path, body, log):
    with open(path, "w") as f:
        f.write(f"#!{sys.executable}\nimport json, sys\nsys.path.insert(0, {ROOT!r})\n{body}\n"
                f"json.dump(doc, open(args.stat, 'w'))\n"
                f"with open({log!r}, 'a') as f:\n    f.write(json.dumps({{'argv': sys.argv[1:], 'stat': doc}}) + '\\n')\n")
    os.chmod(path, 0o755)


def record(script, body, script_args, tmp):
    log = os.path.join(tmp, "calls.jsonl")
    binary = os.path.join(tmp, "stub")
    stub(binary, body, log)
    results = os.path.join(tmp, "results.json")
    argv = [a.format(tmp=tmp, binary=binary, results=results) for a in script_args]
    subprocess.run([sys.executable, script, *argv], check=True, capture_output=True, text=True, timeout=300, cwd=tmp)
    calls = []
    for line in open(log):
        c = json.loads(line)
        a = c["argv"]
        stat = a[a.index("--stat") + 1]
        c["argv"] = ["{stat}" if x == stat else x.replace(tmp, "{tmp}") for x in a]
        calls.append(c)
    return {"script_args": script_args, "calls": calls, "results": json.load(open(results))}


def main():
    ref = os.path.abspath(sys.argv[1])
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        cfgs = []
        for name, doc in SWEEP_CONFIGS.items():
            json.dump(doc, open(os.path.join(tmp, f"{name}.json"), "w"))
            cfgs.append("{tmp}/" + name + ".json")
        out["sweep_scene"] = record(os.path.join(ref, "tools", "sweep_scene.py"), SWEEP_STUB,
                                    ["--viewer-binary", "{binary}", "--scene", "synthetic", "--configs", *cfgs, "--width", "640", "--height", "360",
                                     "--frames", "7", "--iterations", "2", "--timestamp", "--results", "{results}"], tmp)
        out["sweep_scene"]["configs"] = SWEEP_CONFIGS
    with tempfile.TemporaryDirectory() as tmp:
        out["bench_aa"] = record(os.path.join(ref, "tools", "bench_aa.py"), AA_STUB,
                                 ["--binary", "{binary}", "--images", "a.png", "b.png", "--width", "320", "--height", "200", "--frames", "9",
                                  "--iterations", "2", "--results", "{results}"], tmp)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_tools_runs.json")
    json.dump(out, open(path, "w"), indent=1, sort_keys=True)
    print("wrote", path)


if __name__ == "__main__":
    main()
