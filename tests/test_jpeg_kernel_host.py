"""The encoder kernel's own source on the CPU: the device half of csrc/codec/igw_jpeg.hip (everything in front of the
host entry points) compiled as host C++ with a small prelude that supplies what the device supplies -- 256 threads per
workgroup (std::thread) meeting at a std::barrier, LDS as static storage, atomicOr, clz / popcount, and the DPP moves of
the prefix sum with the lane semantics the kernel relies on (row_shr:n inside rows of 16, row_bcast:15 / :31 under a
row mask).  Its streams must equal the numpy model's (tests/jpeg_model.py) byte for byte: the kernel's indexing, its
window rounds, its stuffing and its stride guard are checked without a device, and can be stepped through with a host
debugger.  The GPU run of the same comparison is tests/test_gpu_jpeg.py."""
import os
import subprocess

import numpy as np

import jpeg_model as J
import value_cases as V
from render_checks import LLVM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = os.path.join(LLVM, 'clang++')
GUARD = 0xA5
PRELUDE = r'''#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <thread>
#include <barrier>
#include <vector>
#include <algorithm>
#include "igw_codec.h"
using std::min; using std::max;
#define __shared__ static
#define __constant__
#define __device__
#define __global__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __restrict__
struct Dim { unsigned x; };
static thread_local Dim threadIdx, blockIdx;
static std::barrier<>* g_bar;
#define __syncthreads() g_bar->arrive_and_wait()
static inline void atomicOr(uint32_t* p, uint32_t v) { __atomic_fetch_or(p, v, __ATOMIC_RELAXED); }
static inline int __clz(int v) { return v ? __builtin_clz((unsigned)v) : 32; }
static inline int __popc(uint32_t v) { return __builtin_popcount(v); }
struct uint4 { uint32_t x, y, z, w; };
static int g_x[256];
// emulation of v_mov_dpp semantics as the kernel assumes them (wave = 64 lanes, rows of 16)
static int emu_dpp(int old, int src, int ctrl, int row_mask, int bank_mask, bool bc) {
    int tid = threadIdx.x, lane = tid & 63, wave0 = tid & ~63, row = lane >> 4, lr = lane & 15;
    g_x[tid] = src;
    g_bar->arrive_and_wait();
    int res = old;
    if ((row_mask >> row) & 1) {
        if (ctrl >= 0x111 && ctrl <= 0x11f) { int n = ctrl - 0x110; if (lr >= n) res = g_x[tid - n]; }
        else if (ctrl == 0x142) { if (row > 0) res = g_x[wave0 + 16 * (row - 1) + 15]; }
        else if (ctrl == 0x143) { if (row >= 2) res = g_x[wave0 + 31]; }
        else abort();
    }
    g_bar->arrive_and_wait();
    return res;
}
#define __builtin_amdgcn_update_dpp emu_dpp
'''
MAIN = r'''
}  // namespace
int main(int argc, char** argv) {
    // args: in.raw n W H C quality stride out.raw sizes.raw
    int n = atoi(argv[2]), W = atoi(argv[3]), H = atoi(argv[4]), C = atoi(argv[5]), q = atoi(argv[6]);
    int64_t stride = atoll(argv[7]);
    std::vector<uint8_t> in((size_t)n * W * H * C), out((size_t)n * stride, 0xA5);
    std::vector<int32_t> sizes(n, -7);
    FILE* f = fopen(argv[1], "rb"); if (fread(in.data(), 1, in.size(), f) != in.size()) return 1; fclose(f);
    for (int fr = 0; fr < n; fr++) {
        std::barrier<> bar(256); g_bar = &bar;
        std::vector<std::thread> th;
        for (int t = 0; t < 256; t++) th.emplace_back([&, t] { threadIdx.x = t; blockIdx.x = fr;
            igw_jpeg_encode_kernel(in.data(), W, H, C, q, out.data(), stride, sizes.data()); });
        for (auto& x : th) x.join();
    }
    f = fopen(argv[8], "wb"); fwrite(out.data(), 1, out.size(), f); fclose(f);
    f = fopen(argv[9], "wb"); fwrite(sizes.data(), 4, n, f); fclose(f);
    return 0;
}
'''


def _build(tmp_path):
    src = open(os.path.join(ROOT, 'gridworld_amd', 'csrc', 'codec', 'igw_jpeg.hip')).read()
    body = src[src.index('namespace {'):src.index('thread_local char g_err')]
    cpp, exe = str(tmp_path / 'emu.cpp'), str(tmp_path / 'emu')
    with open(cpp, 'w') as f:
        f.write(PRELUDE + body + MAIN)
    subprocess.check_call([CLANG, '-std=c++20', '-O1', '-pthread', '-I', os.path.join(ROOT, 'include'), '-o', exe, cpp])
    return exe


def _run(exe, tmp_path, frames, quality, stride):
    n, H, W, C = frames.shape
    raw, out, sz = (str(tmp_path / k) for k in ('in.raw', 'out.raw', 'sz.raw'))
    frames.tofile(raw)
    subprocess.check_call([exe, raw, str(n), str(W), str(H), str(C), str(quality), str(stride), out, sz], timeout=120)
    return np.fromfile(out, np.uint8).reshape(n, stride), np.fromfile(sz, np.int32)


def _check(out, sizes, want, stride, what):
    for i in range(len(want)):
        if len(want[i]) <= stride:
            assert sizes[i] == len(want[i]), what + (i,)
            assert out[i, :sizes[i]].tobytes() == want[i], what + (i,)
            assert (out[i, sizes[i]:] == GUARD).all(), what + (i,)
        else:
            assert sizes[i] == -len(want[i]) and out[i].tobytes() == want[i][:stride], what + (i,)


def test_the_kernel_source_on_the_host_equals_the_model_on_every_code_and_at_the_window_boundary(tmp_path):
    """The frames of tests/value_cases.py (pinned by tests/test_value_cases_cpu.py): nearly every AC symbol of both
    tables, 26-bit codes, ZRL chains, blocks without an EOB, every DC category, and the scans that end, or whose chunk
    ends, on the window's last bit.  The three window frames also with a stride a few bytes short of the stream, so
    that the stride guard crosses the aligned flush.  (All of them together take the emulation about ten seconds.)"""
    from gridworld_amd import codec as K
    exe = _build(tmp_path)
    for name, frames, q in V.jpeg_batches():
        want = V.jpeg_streams(name)
        strides = [K.jpeg_bound(frames.shape[2], frames.shape[1])]
        if name in V.aligned():
            strides += [len(want[0]) - 1, len(want[0]) - 5]
        for st in strides:
            out, sizes = _run(exe, tmp_path, np.ascontiguousarray(frames), q, st)
            _check(out, sizes, want, st, (name, q, st))


def test_the_kernel_source_on_the_host_equals_the_model(tmp_path):
    from gridworld_amd import codec as K
    exe = _build(tmp_path)
    rng = np.random.RandomState(1)
    yy, xx = np.mgrid[0:200, 0:328]
    cases = [('noise 64 x 64', rng.randint(0, 256, (2, 64, 64, 3)), (1, 50, 100), None),
             ('noise 96 x 40', rng.randint(0, 256, (1, 40, 96, 3)), (90,), None),
             ('noise 13 x 7 rgba', rng.randint(0, 256, (2, 7, 13, 4)), (75,), None),
             ('1 x 1', rng.randint(0, 256, (2, 1, 1, 3)), (90,), None),
             ('flat', np.stack([np.full((16, 24, 3), v) for v in (0, 255, 77)]), (100, 40), None),
             # 255 MCUs: four chunks, the last one short; at quality 100 a chunk of noise takes several windows
             ('noise 136 x 120', rng.randint(0, 256, (1, 120, 136, 3)), (100, 30), None),
             ('smooth 328 x 200 rgba', np.stack([(xx * 3 + yy) % 256, (yy * 2) % 256, (xx + yy * yy // 64) % 256,
                                                 xx % 256], -1)[None], (90,), None),
             ('a stride too small', rng.randint(0, 256, (2, 64, 64, 3)), (95,), 2048)]
    for what, f, qualities, stride in cases:
        f = np.ascontiguousarray(f.astype(np.uint8))
        st = stride or K.jpeg_bound(f.shape[2], f.shape[1])
        for q in qualities:
            out, sizes = _run(exe, tmp_path, f, q, st)
            _check(out, sizes, [J.encode(x, q) for x in f], st, (what, q))
