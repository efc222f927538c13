"""DevBuf<T> (gravo_mg_amd/csrc/dev_buf.hpp), the owner of every pool-backed device array of the engine, without a device: the header
includes nothing of HIP and releases through one hook, which a stand-alone program built with AddressSanitizer + UBSan defines as a recorder.
Pointers are made-up addresses that nobody dereferences."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_MAIN = r"""
#include <cstdint>
#include <cstdio>
#include <map>
#include <type_traits>
#include <vector>
#include "dev_buf.hpp"

static std::map<void*, int> released;                   // the recording stub: how often every address was handed to the hook
static std::vector<void*> order;
void dev_buf_release(void* p) { ++released[p]; order.push_back(p); }

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { if (fails < 20) std::printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

static uintptr_t next_addr = 0x1000;
template <class T> T* fresh() { next_addr += 0x100; return reinterpret_cast<T*>(next_addr); }
static int times(void* p) { auto it = released.find(p); return it == released.end() ? 0 : it->second; }
static size_t total() { return order.size(); }

static_assert(!std::is_copy_constructible_v<DevBuf<int>> && !std::is_copy_assignable_v<DevBuf<int>>, "one owner");
static_assert(std::is_nothrow_move_constructible_v<DevBuf<int>> && std::is_nothrow_move_assignable_v<DevBuf<int>>, "moves");

struct Holder {                                         // several buffers and plain members, like the engine's Level
    int n = 0;
    DevBuf<double> x, b;
    DevBuf<int> idx;
    DevBuf<float> x32;
};
static_assert(!std::is_copy_constructible_v<Holder> && std::is_nothrow_move_constructible_v<Holder>, "a struct of buffers moves, never copies");

int main() {
    {   // empty by default: nothing to release
        DevBuf<int> e;
        EXPECT(e.get() == nullptr && !e && !e.borrowed());
    }
    EXPECT(total() == 0);
    int* a = fresh<int>();
    {   // released exactly once, by the destructor; reads like a pointer meanwhile
        DevBuf<int> v;
        v.adopt(a);
        int* as_pointer = v;
        EXPECT(as_pointer == a && v.get() == a && v + 3 == a + 3 && v != nullptr && !v.borrowed());
    }
    EXPECT(times(a) == 1 && total() == 1);
    int *b = fresh<int>(), *c = fresh<int>();
    {   // a moved-from buffer releases nothing; move assignment releases the target's old block first
        DevBuf<int> v, w;
        v.adopt(b); w.adopt(c);
        DevBuf<int> u(std::move(v));
        EXPECT(v.get() == nullptr && u.get() == b && times(b) == 0);
        u = std::move(w);
        EXPECT(times(b) == 1 && order.back() == b && w.get() == nullptr && u.get() == c && times(c) == 0);
        u = std::move(u);                               // (self-assignment keeps the block)
        EXPECT(u.get() == c && times(c) == 0);
        v = DevBuf<int>();                              // "assign an empty one" on an empty one
        EXPECT(total() == 2);
    }
    EXPECT(times(b) == 1 && times(c) == 1 && total() == 3);
    int *d = fresh<int>(), *d2 = fresh<int>();
    {   // reset() is idempotent; adopt releases what was held
        DevBuf<int> v;
        v.adopt(d);
        v.reset(); v.reset();
        EXPECT(times(d) == 1 && v.get() == nullptr);
        v.adopt(d2); v.adopt(d);
        EXPECT(times(d2) == 1 && times(d) == 1);
        v = {};
        EXPECT(times(d) == 2 && total() == 6);
    }
    EXPECT(total() == 6);
    double *ext = fresh<double>(), *own = fresh<double>(), *own2 = fresh<double>();
    {   // a borrowed pointer never reaches the hook: not from the destructor, reset(), move assignment (either side) or a re-borrow
        { DevBuf<double> v; v.borrow(ext); EXPECT(v.borrowed() && v.get() == ext); }
        { DevBuf<double> v; v.borrow(ext); v.reset(); EXPECT(!v.borrowed() && v.get() == nullptr); }
        { DevBuf<double> v, w; v.borrow(ext); w.adopt(own); v = std::move(w); EXPECT(!v.borrowed() && v.get() == own && times(own) == 0); }
        EXPECT(times(own) == 1);
        {   // the bind / unbind of level 0: park the owner by move, borrow, move the owner back
            DevBuf<double> level, parked;
            level.adopt(own2);
            parked = std::move(level);
            level.borrow(ext);
            EXPECT(level.borrowed() && level.get() == ext && parked.get() == own2);
            DevBuf<double> moved(std::move(level));         // the state travels with a move (a vector of levels that grows)
            EXPECT(moved.borrowed() && !level.borrowed() && level.get() == nullptr);
            level = std::move(moved);
            level.borrow(ext);                              // bound again while bound
            level = std::move(parked);
            EXPECT(!level.borrowed() && level.get() == own2 && times(own2) == 0);
        }
        EXPECT(times(own2) == 1 && times(ext) == 0);
        { DevBuf<double> v; v.adopt(own); v.borrow(ext); EXPECT(times(own) == 2); }       // borrowing over an owned block releases that block
        EXPECT(times(ext) == 0);
    }
    {   // a vector of holders: every block once, over growth (reallocation moves the elements), resize and clear
        released.clear(); order.clear();
        std::vector<void*> made;
        auto fill = [&](Holder& h, int n) {
            h.n = n;
            double *x = fresh<double>(), *bb = fresh<double>();
            int* i = fresh<int>();
            h.x.adopt(x); h.b.adopt(bb); h.idx.adopt(i);   // (x32 stays empty, like the fp32 twins of an fp64 handle)
            made.push_back(x); made.push_back(bb); made.push_back(i);
        };
        std::vector<Holder> lv;
        for (int k = 0; k < 9; ++k) { lv.emplace_back(); fill(lv.back(), k); }       // grows through several capacities
        EXPECT(total() == 0);
        for (int k = 0; k < 9; ++k) EXPECT(lv[k].n == k && lv[k].x.get() == made[3 * k]);
        lv.resize(4);
        EXPECT(total() == 15);
        lv.resize(12);                                   // empty holders at the end, the first four moved or kept
        EXPECT(total() == 15 && lv[3].idx.get() == made[11] && lv[11].x.get() == nullptr);
        lv[1] = {};                                      // releasing a structure is assigning an empty one
        EXPECT(total() == 18 && times(made[3]) == 1 && times(made[4]) == 1 && times(made[5]) == 1);
        fill(lv[10], 10);
        lv.clear();
        EXPECT(total() == made.size());
        for (void* p : made) EXPECT(times(p) == 1);
    }
    std::printf(fails ? "%d checks failed\n" : "all checks passed\n", fails);
    return fails ? 1 : 0;
}
"""


def test_one_owner_per_block_under_address_and_ub_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src = tmp_path / "dev_buf_main.cpp"
    src.write_text(_MAIN)
    exe = tmp_path / "dev_buf_main"
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wno-self-move", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", os.path.join(ROOT, "gravo_mg_amd", "csrc"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and "all checks passed" in run.stdout, run.stdout + run.stderr
