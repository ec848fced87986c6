"""How the tests build and run host code: one compiler line for stand-alone programs, one for the libraries ctypes loads, one way to run a
program, and the C-against-ctypes layout check.

A stand-alone program (its own main) is the only sanitized form: it is built with the sanitizers and run directly, with nothing preloaded.
A library loaded into Python is never instrumented -- the interpreter is not, so the sanitizer's runtime would have to be preloaded -- and
build_library refuses a -fsanitize flag.  Code that a test loads through ctypes and wants under the sanitizers gets a main of its own
(tests/cpp/cacao_core_host.cpp -DCACAO_HOST_MAIN is one)."""
import os
import subprocess
from collections import namedtuple

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
INCLUDE = os.path.join(ROOT, "include")
BASE = ["-O1", "-g", "-Wall", "-Werror"]
EXACT = ["-ffp-contract=off"]
SANITIZERS = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


def product(lib_dir="lib"):
    """`extra` for a program that drives the built libraries (granite_amd/<lib_dir>) as an integrator would"""
    lib = os.path.join(ROOT, "granite_amd", lib_dir)
    return ["-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + INCLUDE, "-L" + lib, "-lgranite_host", "-lgranite_hip", "-Wl,-rpath," + lib,
            "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"]


PRODUCT = product()

ProgramFixtures = namedtuple("ProgramFixtures", "plain sanitized")


def _sources(sources):
    """one name or several; a bare name lies in tests/cpp"""
    return [os.path.join(CPP, s) for s in ([sources] if isinstance(sources, str) else sources)]


def _compile(out, sources, std, exact, flags, extra):
    # `extra` comes last: an -O2 in it overrides the base's -O1, and -l flags follow the sources that need them
    subprocess.check_call(["g++", *BASE, f"-std={std}", *(EXACT if exact else []), *flags, "-o", str(out), *_sources(sources), *extra])
    return str(out)


def build_program(directory, name, sources, *, sanitized=False, std="c++17", exact=False, extra=()):
    """Build a stand-alone program from `sources` into directory/name and return its path.  exact=True forbids contraction;
    sanitized=True builds it with the address and undefined-behaviour sanitizers, to be run directly with nothing preloaded."""
    return _compile(os.path.join(directory, name), sources, std, exact, SANITIZERS if sanitized else [], extra)


def build_library(directory, name, sources, *, std="c++17", exact=False, extra=()):
    """Build a shared library for ctypes into directory/name and return its path.  Never with a sanitizer (see the module's docstring)."""
    if any(flag.startswith("-fsanitize") for flag in extra):
        raise ValueError("a library loaded into Python is not instrumented: give the code a main and use build_program(sanitized=True)")
    return _compile(os.path.join(directory, name), sources, std, exact, ["-shared", "-fPIC"], extra)


def run_program(exe, *args, input_bytes=None, tmp_path=None, timeout=600):
    """Run exe with args and return its stdout as bytes; input_bytes go to tmp_path/case.bin, whose path becomes the last argument.  A
    non-zero exit fails the test with the status and the end of stderr.  The environment is the caller's, untouched."""
    args = [str(a) for a in args]
    if input_bytes is not None:
        case = tmp_path / "case.bin"
        case.write_bytes(input_bytes)
        args.append(str(case))
    r = subprocess.run([str(exe), *args], capture_output=True, timeout=timeout)
    if r.returncode != 0:
        pytest.fail(f"{os.path.basename(str(exe))} exited with status {r.returncode}:\n{r.stderr[-3000:].decode(errors='replace')}", pytrace=False)
    return r.stdout


def program_fixtures(sources, *, name=None, **build_options):
    """The module-scoped fixtures (plain, sanitized): the program of `sources`, built on first use in a directory of its own."""
    name = name or os.path.splitext(os.path.basename(_sources(sources)[0]))[0]

    def fixture(sanitized):
        suffix = "_san" if sanitized else ""

        @pytest.fixture(scope="module")
        def program(tmp_path_factory):
            return build_program(tmp_path_factory.mktemp(name + suffix), name + suffix, sources, sanitized=sanitized, **build_options)
        return program
    return ProgramFixtures(fixture(False), fixture(True))


def c_layout(tmp_path, c_type, fields, header="granite_hip.h"):
    """[sizeof(c_type), offsetof(c_type, field)...] as a C11 compiler lays `header`'s structure out"""
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(f'#include "{header}"\n#include <stdio.h>\n#include <stddef.h>\nint main(void) {{\n  printf("%zu\\n", sizeof({c_type}));\n' +
                   "".join(f'  printf("%zu\\n", offsetof({c_type}, {f}));\n' for f in fields) + "  return 0;\n}\n")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", INCLUDE, "-o", str(exe), str(src)])
    return [int(v) for v in run_program(exe).split()]
