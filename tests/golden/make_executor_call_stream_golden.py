"""Generates tests/golden/executor_call_stream_parent.json: what the executor asks of the HIP runtime, call by call.

tests/hip_stub prints under HIP_STUB_TRACE=1 every launch (L), event record (R), stream wait (W), event query (Q), host wait (S) and
graph launch (G) with its stream and event.  The committed file was recorded with the host library of the commit BEFORE stream planning
and cross-stream hazard tracking moved from render_graph.cpp into frame_schedule.cpp; tests/test_executor_call_stream_cpu.py holds every
later library to it.  Do not regenerate it to make that test pass: a changed line is a changed wait, record, query or skip.

The normal form of one case (everything behind its "=== case" line): streams and events renumbered by first appearance, a run of
consecutive launches on one stream collapsed to one "L s<k>" (fusing kernels does not touch the fixture), "[sync]" lines of
GRANITE_SYNC_DEBUG=1 kept as they are.  Next to it, of every graph the case baked: stream per pass, double_buffered and alias_of per resource.

    python tests/golden/make_executor_call_stream_golden.py [--lib-dir lib_xyz]      # records twice, requires equality, writes the file

CASES, record() and record_all() are what the test imports."""
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "executor_call_stream_parent.json")
STUB = os.path.join(ROOT, "tests", "hip_stub", "libhip_stub.so")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import host_program  # noqa: E402

APP_WORKER = r'''
import json, sys
sys.path.insert(0, %(root)r)
import numpy as np
from granite_amd import app as gapp, synth
name, lights = sys.argv[1], int(sys.argv[2])
if name == "post_only":
    a = gapp.Application(256, 256, lighting=False); a.upload_hdr(synth.make_hdr(256, 256))
else:
    w, h = 512, 288
    cam = synth.Camera(w, h)
    kw = {"plain": {}, "fxaa": dict(post_aa=gapp.POST_AA_FXAA), "taa_smaa": dict(pre_aa=gapp.POST_AA_TAA_HIGH, post_aa=gapp.POST_AA_SMAA_ULTRA)}[name]
    a = gapp.Application(w, h, lighting=True, hdr_bloom=True, dynamic_exposure=True, compute_post=True, **kw)
    if "pre_aa" in kw:
        a.set_camera(np.ascontiguousarray(cam.P.T, np.float32).reshape(16), np.ascontiguousarray(cam.V.T, np.float32).reshape(16))
    else:
        a.set_render_parameters(cam.render_params())
    a.set_lights(synth.make_lights(cam, lights))
    a.upload_gbuffer(synth.make_gbuffer(cam), synth.make_motion_vectors(w, h) if "pre_aa" in kw else None)
sys.stderr.write("=== case %%s frames\n=== graph %%s\n" %% (name, json.dumps(a.graph()))); sys.stderr.flush()
a.render_frames(8, sync=False)
a.render_frames(2, sync=True)
a.close()
'''

# name -> (what runs, environment on top of HIP_STUB_TRACE=1).  Lights stay below 1000: above, the light refresh moves to helper threads.
PENDING = {"HIP_STUB_EVENTS_PENDING": "1"}  # a recorded event never reads as complete: every dependency the host cannot rule out is a wait
CASES = {"execute40_pending": (("execute", 40), PENDING),
         # the same generator with a backbuffer source that is not the swapchain's format and is written on the async compute stream: every
         # frame ends in the final blit, which waits for that stream and publishes its read under an event of its own
         "execute_blit12_pending": (("execute-blit", 12), PENDING)}
for _graph in ("post_only", "plain", "fxaa", "taa_smaa"):
    CASES[_graph] = (("app", _graph, 300), {})
    CASES[_graph + "_pending"] = (("app", _graph, 300), PENDING)
# above 512 lights the cluster front no longer reads the staged light arrays itself: the upload launch runs
CASES["plain_600_lights"] = (("app", "plain", 600), {})
CASES["plain_600_lights_pending"] = (("app", "plain", 600), PENDING)
for _switch, _value in (("GRANITE_ALTERNATE_FRONT", "1"), ("GRANITE_HOST_LEAD_FRAMES", "3"), ("GRANITE_SPLIT_TAIL", "0"), ("GRANITE_SYNC_DEBUG", "1"),
                        ("GRANITE_LAUNCH_GRAPHS", "1")):
    CASES["taa_smaa_pending_%s" % _switch.lower()] = (("app", "taa_smaa", 300), dict(PENDING, **{_switch: _value}))

TRACE_LINE = re.compile(r"^([LRWQSG]) (s\d+)(?: (e\d+))?(?: .*)?$")
SWITCHES = ("GRANITE_ALTERNATE_FRONT", "GRANITE_HOST_LEAD_FRAMES", "GRANITE_SPLIT_TAIL", "GRANITE_SYNC_DEBUG", "GRANITE_LAUNCH_GRAPHS",
            "GRANITE_STREAM_PRIORITIES", "GRANITE_UNSAFE_NO_CROSS_SYNC", "GRANITE_SYNC_EVENT_SYSTEM_FENCE", "GRANITE_LIGHT_PREFETCH_MIN",
            "HIP_STUB_EVENTS_PENDING")


def normal_form(lines):
    streams, events, out = {}, {}, []
    for line in lines:
        if line.startswith("[sync]"):
            out.append(line)
            continue
        m = TRACE_LINE.match(line)
        if not m:
            continue
        what, stream, event = m.groups()
        text = "%s s%d" % (what, streams.setdefault(stream, len(streams)))
        if event:
            text += " e%d" % events.setdefault(event, len(events))
        if what == "L" and out and out[-1] == text:
            continue
        out.append(text)
    return out


def graph_summary(doc):
    return {"streams": [[p["name"], p["stream"]] for p in doc["passes"]],
            "resources": [[r["name"], r["double_buffered"], r["alias_of"]] for r in doc["resources"]]}


def split_cases(stderr):
    """{"<case name>": {"calls": normal form, "graph": summary}} for every "=== case" section of a trace."""
    out = {}
    for chunk in stderr.split("=== case ")[1:]:
        lines = chunk.splitlines()
        graph = [l for l in lines[1:] if l.startswith("=== graph ")]
        assert len(graph) == 1, lines[0]
        assert lines[0] not in out, lines[0]
        out[lines[0]] = {"calls": normal_form(lines[1:]), "graph": graph_summary(json.loads(graph[0][len("=== graph "):]))}
    return out


def build_tools(lib_dir, scratch):
    if not os.path.exists(STUB) or os.path.getmtime(STUB) < os.path.getmtime(os.path.join(os.path.dirname(STUB), "hip_stub.cpp")):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(STUB)])
    return host_program.build_program(scratch, "graph_cases", "graph_cases.cpp", extra=host_program.product(lib_dir))


def record(name, exe, lib_dir="lib"):
    what, extra = CASES[name]
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(LD_PRELOAD=STUB, HIP_STUB_TRACE="1", GRANITE_LIB_DIR=lib_dir, **extra)
    if what[0] != "app":
        command = [exe, "--" + what[0], str(what[1])]
    else:
        command = [sys.executable, "-c", APP_WORKER % {"root": ROOT}, what[1], str(what[2])]
    r = subprocess.run(command, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (name, r.stdout[-1000:], r.stderr[-3000:])
    sections = split_cases(r.stderr)
    assert sections, (name, r.stderr[-3000:])
    return sections


def record_all(lib_dir="lib", names=None):
    with tempfile.TemporaryDirectory() as scratch:
        exe = build_tools(lib_dir, scratch)
        return {name: record(name, exe, lib_dir) for name in (names or CASES)}


if __name__ == "__main__":
    lib_dir = sys.argv[sys.argv.index("--lib-dir") + 1] if "--lib-dir" in sys.argv else "lib"
    first, second = record_all(lib_dir), record_all(lib_dir)
    unstable = [name for name in CASES if first[name] != second[name]]
    assert not unstable, "not reproducible, drop by name and say why: %s" % unstable
    with open(PATH, "w") as f:
        json.dump(first, f, separators=(",", ":"))
        f.write("\n")
    lines = {name: sum(len(s["calls"]) for s in sections.values()) for name, sections in first.items()}
    print(json.dumps({"cases": len(first), "graphs": sum(len(s) for s in first.values()), "lines": lines, "bytes": os.path.getsize(PATH)}))
