"""csrc/dispatch.h turns a run-time integer into a template argument for every launcher (which kernel instantiation a value reaches is
behaviour: a wrong one can compute the right numbers and only be slower).  The header is plain C++17, so a stand-alone g++ program -
AddressSanitizer + UndefinedBehaviorSanitizer on, it is an ordinary executable - walks it: every listed value, unlisted values on every side,
the strict form's refusal, a three-deep nest and the return value's way back."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GXX = shutil.which("g++")

PROGRAM = r"""
#include <climits>
#include <cstdio>
#include <set>
#include <string>
#include <tuple>

#include "dispatch.h"

using stego::with_const;
using stego::with_const_or;

static int failures = 0;
#define CHECK(...) do { if (!(__VA_ARGS__)) { std::printf("FAILED line %d: %s\n", __LINE__, #__VA_ARGS__); ++failures; } } while (0)

enum Err { OK = 0, INVALID = 1 };           // stands in for hipSuccess / hipErrorInvalidValue

int main()
{
    const int unlisted[] = {INT_MIN, -1, 0, 4, 6, 9, 100, INT_MAX};        // below, between and above the listed 1, 2, 3, 5, 8
    // the permissive form: a listed value reaches its own constant, anything else the last one; f runs exactly once
    for (int v : {1, 2, 3, 5, 8}) {
        int calls = 0;
        const int got = with_const<1, 2, 3, 5, 8>(v, [&](auto N) { ++calls; return (int)N(); });
        CHECK(got == v && calls == 1);
    }
    for (int v : unlisted) {
        int calls = 0;
        const int got = with_const<1, 2, 3, 5, 8>(v, [&](auto N) { ++calls; return (int)N(); });
        CHECK(got == 8 && calls == 1);
    }
    {   // one listed value takes everything; negative constants are constants too
        int calls = 0;
        CHECK(with_const<7>(INT_MIN, [&](auto N) { ++calls; return (int)N(); }) == 7 && calls == 1);
        CHECK(with_const<-1, 4, 2, 0>(-1, [](auto N) { return (int)N(); }) == -1);
        CHECK(with_const<-1, 4, 2, 0>(3, [](auto N) { return (int)N(); }) == 0);
    }
    // the strict form: listed values as above, an unlisted one gets `otherwise` back and f is not called
    for (int v : {1, 2, 3, 5, 8}) {
        int calls = 0, seen = -1;
        const Err e = with_const_or<1, 2, 3, 5, 8>(v, INVALID, [&](auto N) { ++calls; seen = N(); return OK; });
        CHECK(e == OK && calls == 1 && seen == v);
    }
    for (int v : unlisted) {
        int calls = 0;
        const Err e = with_const_or<1, 2, 3, 5, 8>(v, INVALID, [&](auto) { ++calls; return OK; });
        CHECK(e == INVALID && calls == 0);
    }
    {   // the constant is a compile-time value inside f: it sizes an array
        const size_t n = with_const<2, 3, 4>(3, [](auto N) { char a[N() * 10]; return sizeof(a); });
        CHECK(n == 30);
    }
    {   // three deep, as the fused forward's launchers nest it: {0, 1} x {384, 768} x {1, 2, 3, 4} -> 16 distinct triples, each its own
        std::set<std::tuple<int, int, int>> seen;
        int calls = 0;
        for (int p : {0, 1})
            for (int c : {384, 768})
                for (int k : {1, 2, 3, 4}) {
                    const auto t = with_const<0, 1>(p, [&](auto P) {
                        return with_const<384, 768>(c, [&](auto C) {
                            return with_const<1, 2, 3, 4>(k, [&](auto K) { ++calls; return std::make_tuple((int)P(), (int)C(), (int)K()); });
                        });
                    });
                    CHECK(t == std::make_tuple(p, c, k));
                    seen.insert(t);
                }
        CHECK(seen.size() == 16 && calls == 16);
        // and a strict level under two permissive ones refuses without reaching the innermost f
        int inner = 0;
        const Err e = with_const<0, 1>(5, [&](auto) {
            return with_const<384, 768>(192, [&](auto) { return with_const_or<2, 3, 4>(1, INVALID, [&](auto) { ++inner; return OK; }); });
        });
        CHECK(e == INVALID && inner == 0);
    }
    {   // whatever f returns comes back unchanged: a value of another type, a reference, nothing
        const std::string s = with_const<1, 2>(2, [](auto N) { return std::string("n") + std::to_string(N()); });
        CHECK(s == "n2");
        int slots[3] = {0, 0, 0};
        int& r = with_const<0, 1, 2>(1, [&](auto N) -> int& { return slots[N()]; });
        r = 42;
        CHECK(slots[1] == 42 && &r == &slots[1]);
        int hits = 0;
        with_const<1, 2>(1, [&](auto N) { hits += N(); });
        CHECK(hits == 1);
    }
    if (!failures) std::printf("dispatch ok\n");
    return failures ? 1 : 0;
}
"""


@pytest.mark.skipif(GXX is None, reason="needs g++")
def test_with_const_reaches_the_listed_constants(tmp_path):
    src = tmp_path / "dispatch_main.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "dispatch_main"
    cmd = [GXX, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "stego_amd", "csrc"), str(src), "-o", str(exe)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and "dispatch ok" in run.stdout, (run.stdout + run.stderr)[-3000:]
