"""CPU: tests/host_program.py, which builds and runs the host programs of the other tests.  A failing program fails the test with its
exit status and what it wrote to stderr; the sanitized build really is instrumented and the plain one is not (the program says which it
is: it is built with the sanitizers and run directly, nothing is preloaded, and nothing is made to fault); a library for ctypes is never
built with a sanitizer; and c_layout gives what ctypes gives for gr_image."""
import ctypes as C

import pytest

from granite_amd import capi
from host_program import build_library, build_program, c_layout, run_program

EXITS_3 = '#include <cstdio>\nint main() { std::fputs("marker-7f3a on stderr\\n", stderr); return 3; }\n'
SAYS_WHETHER_SANITIZED = """#include <cstdio>
int main() {
#if defined(__SANITIZE_ADDRESS__)
    std::puts("yes");
#else
    std::puts("no");
#endif
    return 0;
}
"""


def write(tmp_path, name, text):
    path = tmp_path / name
    path.write_text(text)
    return str(path)


def test_a_failing_program_fails_the_test_with_its_status_and_stderr(tmp_path):
    exe = build_program(tmp_path, "exits_3", write(tmp_path, "exits_3.cpp", EXITS_3))
    with pytest.raises(pytest.fail.Exception) as failure:
        run_program(exe)
    assert "status 3" in str(failure.value) and "marker-7f3a on stderr" in str(failure.value)


@pytest.mark.parametrize("sanitized, answer", [(False, b"no\n"), (True, b"yes\n")], ids=["plain", "sanitized"])
def test_the_sanitized_build_is_instrumented_and_the_plain_one_is_not(tmp_path, sanitized, answer):
    exe = build_program(tmp_path, "says", write(tmp_path, "says.cpp", SAYS_WHETHER_SANITIZED), sanitized=sanitized)
    assert run_program(exe) == answer


def test_input_bytes_arrive_as_a_file_named_last(tmp_path):
    echo = '#include <cstdio>\nint main(int argc, char **argv) { std::FILE *f = std::fopen(argv[argc - 1], "rb"); int c; while ((c = std::fgetc(f)) != EOF) std::putchar(c); return argc == 3 ? 0 : 1; }\n'
    exe = build_program(tmp_path, "echo", write(tmp_path, "echo.cpp", echo))
    assert run_program(exe, "first", input_bytes=b"\x00\xffabc", tmp_path=tmp_path) == b"\x00\xffabc"


def test_a_library_for_ctypes_is_never_sanitized(tmp_path):
    source = write(tmp_path, "answer.cpp", 'extern "C" int answer() { return 42; }\n')
    with pytest.raises(ValueError, match="not instrumented"):
        build_library(tmp_path, "libanswer.so", source, extra=["-fsanitize=address"])
    assert C.CDLL(build_library(tmp_path, "libanswer.so", source)).answer() == 42


def test_c_layout_of_gr_image_is_the_ctypes_one(tmp_path):
    fields = [name for name, _ in capi.Image._fields_]
    assert c_layout(tmp_path, "gr_image", fields) == [C.sizeof(capi.Image)] + [getattr(capi.Image, f).offset for f in fields]
