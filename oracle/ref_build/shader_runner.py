"""The recipe the golden makers (tests/golden/make_*_golden.py) share for executing the reference's code on the CPU: re-spell its GLSL with
gen_swizzles.py and glsl2cpp.py into a scratch directory, compile a runner against glsl_cpu.hpp once per specialisation, compile what the
runner needs of the reference's math library from where it lies, link a library for ctypes, and remove the directory.  The recipe only:
the reference's text is read from REF, what is compiled from it lives in the scratch directory and goes with it."""
import contextlib
import os
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("REF", "/root/reference")  # as the Makefile's
SHADERS = os.path.join(REF, "assets", "shaders")
MATH = os.path.join(REF, "math")
MUGLM = os.path.join(MATH, "muglm", "muglm.cpp")
RUNNER_FLAGS = ["-O2", "-std=c++20", "-fPIC", "-ffp-contract=off", "-w", "-I" + HERE]
MATH_FLAGS = ["-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-msse4.1", "-w", "-I" + MATH, "-I" + os.path.join(REF, "util")]


@contextlib.contextmanager
def scratch(prefix):
    """a temporary directory, removed on exit whatever happened inside"""
    tmp = tempfile.mkdtemp(prefix=prefix)
    try:
        yield tmp
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def respell(gen_dir, shaders, patch=None):
    """gen_dir/<shader's base name>.inc for every shader (a path, relative ones under SHADERS), next to the swizzle tables.  `patch` edits
    the .inc text where the re-spelling needs help: one callable for every shader, or {shader: callable} for some."""
    os.makedirs(gen_dir)
    subprocess.check_call([sys.executable, os.path.join(HERE, "gen_swizzles.py"), gen_dir])
    for shader in shaders:
        inc = os.path.join(gen_dir, os.path.splitext(os.path.basename(shader))[0] + ".inc")
        subprocess.check_call([sys.executable, os.path.join(HERE, "glsl2cpp.py"), os.path.join(SHADERS, shader), inc])
        fix = patch.get(shader) if isinstance(patch, dict) else patch
        if fix:
            with open(inc) as f:
                text = f.read()
            with open(inc, "w") as f:
                f.write(fix(text))


def compile_objects(tmp, flags, sources, jobs=1):
    """tmp/<name>.o for every (name, source, defines), `jobs` compilers at a time; returns the objects in order"""
    commands = [["g++", *flags, *defines, "-c", source, "-o", os.path.join(tmp, name + ".o")] for name, source, defines in sources]
    with ThreadPoolExecutor(jobs) as pool:
        list(pool.map(subprocess.check_call, commands))
    return [c[-1] for c in commands]


def compile_runner(tmp, runner, variants, extra=(), jobs=1):
    """the runner against glsl_cpu.hpp and tmp/gen, once per (object name, defines)"""
    return compile_objects(tmp, [*RUNNER_FLAGS, "-I" + tmp, *extra], [(name, runner, defines) for name, defines in variants], jobs)


def reference_math_objects(tmp, sources, extra=()):
    """(name, source, defines) compiled as the reference's math library needs it: muglm.cpp, transforms.cpp or aabb.cpp from REF, and a
    runner's part that calls them"""
    return compile_objects(tmp, [*MATH_FLAGS, *extra], sources)


def link(lib, objects, extra=()):
    subprocess.check_call(["g++", "-shared", *extra, "-o", lib, *objects])
    return lib
