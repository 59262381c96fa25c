"""csrc/ws_layout.h carves every add-on unit's workspace: plan() takes the regions in order and keeps the offsets, the launcher turns an
offset into a typed pointer.  The header is plain C++17, so a stand-alone g++ program that includes it alone walks both alignment styles
in use - every region on its own 16 bytes, and regions packed tight with only the size rounded to 8 - against the chains of
`o = up16(o + n)` and `o += n` they replaced, zero-byte regions included.  It runs twice: as built, and with AddressSanitizer +
UndefinedBehaviorSanitizer on (an ordinary executable: no device, nothing preloaded)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GXX = shutil.which("g++")

PROGRAM = r"""
#include <cstdint>
#include <cstdio>
#include <vector>

#include "ws_layout.h"

using stego::WsLayout;

static int failures = 0;
#define CHECK(...) do { if (!(__VA_ARGS__)) { std::printf("FAILED line %d: %s\n", __LINE__, #__VA_ARGS__); ++failures; } } while (0)

static size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

int main()
{
    {   // nothing taken
        WsLayout l;
        CHECK(l.total(1) == 0 && l.total(8) == 0 && l.total(16) == 0);
    }
    {   // every region on its own 16 bytes: the offsets and the size of the chain o = up16(o + n), for sizes on every side of a multiple
        const size_t sizes[] = {1, 0, 15, 16, 17, 0, 0, 4, 8, 12, 31, 32, 33, 4096, 1, 9397204976ull, 3, 0};
        WsLayout l;
        size_t o = 0;
        for (size_t n : sizes) {
            CHECK(l.take(n, 16) == o);
            CHECK(o % 16 == 0);
            o = up16(o + n);
            CHECK(l.total(16) == o);
        }
    }
    {   // a zero-byte region shares its offset with the next one and moves nothing
        WsLayout l;
        const size_t a = l.take(48, 16), b = l.take(0, 16), c = l.take(20, 16), d = l.take(0, 16);
        CHECK(a == 0 && b == 48 && c == 48 && d == 80 && l.total(16) == 80);
    }
    {   // packed tight, the size rounded to 8: the chain o += n, the first region at 0 whatever its name
        const size_t sizes[] = {24, 100, 0, 12, 12, 0, 4, 1, 3};
        WsLayout l;
        size_t o = 0;
        for (size_t n : sizes) {
            CHECK(l.take(n, 1) == o);
            o += n;
            CHECK(l.total(8) == ((o + 7) & ~(size_t)7));
            CHECK(l.total(1) == o);
        }
        CHECK(l.total(8) == 160);
    }
    {   // the two styles mix: an aligned region after packed ones starts on its boundary
        WsLayout l;
        CHECK(l.take(5, 1) == 0 && l.take(3, 4) == 8 && l.take(1, 16) == 16 && l.take(2, 1) == 17 && l.total(8) == 24);
    }
    {   // at<T>: the typed pointer of a region, usable over its whole length
        WsLayout l;
        const size_t off_d = l.take(3 * sizeof(double), 16), off_f = l.take(5 * sizeof(float), 16), off_b = l.take(7, 16);
        std::vector<unsigned char> raw(l.total(16) + 16);
        void* ws = raw.data() + (16 - reinterpret_cast<uintptr_t>(raw.data()) % 16) % 16;
        double* d = stego::at<double>(ws, off_d);
        float* f = stego::at<float>(ws, off_f);
        unsigned char* b = stego::at<unsigned char>(ws, off_b);
        CHECK(reinterpret_cast<unsigned char*>(d) == static_cast<unsigned char*>(ws) + off_d);
        CHECK(reinterpret_cast<uintptr_t>(f) % 16 == 0 && reinterpret_cast<unsigned char*>(f) == static_cast<unsigned char*>(ws) + 32);
        for (int i = 0; i < 3; ++i) d[i] = 1.5 * i;
        for (int i = 0; i < 5; ++i) f[i] = 2.f * i;
        for (int i = 0; i < 7; ++i) b[i] = (unsigned char)i;
        CHECK(d[2] == 3.0 && f[4] == 8.f && b[6] == 6 && off_b == 64 && l.total(16) == 80);
        const void* cws = ws;
        CHECK(stego::at<const float>(const_cast<void*>(cws), off_f)[1] == 2.f);
    }
    if (!failures) std::printf("ws_layout ok\n");
    return failures ? 1 : 0;
}
"""


@pytest.mark.skipif(GXX is None, reason="needs g++")
@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_ws_layout_offsets_and_totals(tmp_path, sanitize):
    src = tmp_path / "ws_layout_main.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "ws_layout_main"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    cmd = [GXX, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra"] + flags + ["-I", os.path.join(ROOT, "stego_amd", "csrc"), str(src), "-o", str(exe)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and "ws_layout ok" in run.stdout, (run.stdout + run.stderr)[-3000:]
