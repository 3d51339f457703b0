#!/usr/bin/env python
"""The decode kernels of csrc/jpegdec.hip run on the CPU: the kernel source (everything in front of its host section) is compiled as HOST
code behind a small shim (threadIdx / blockIdx as globals, one lane at a time) into a stand-alone program with AddressSanitizer and UBSan,
and run over every fixture of tests/golden/jpeg_u8.npz, a mixed batch and cut segments.  It checks the entropy, inverse-DCT and colour
kernels' arithmetic and every index they form (out-of-bounds reads or writes abort the program); the scan kernel's wave-level marker search
is replaced by a serial loop, so that kernel is covered on the GPU only.  Needs a clang++ that knows ext_vector_type (ROCm's will do) and
no GPU.

The sync entropy mode is covered through its one-subsequence device function, jpeg_sub_decode: a plain host loop drives it through the
rounds, the scan and the write pass exactly as jpeg_entropy_sync_kernel does (same entry rules, same change flags, same skips), over every
fixture without restart markers at 16, 32 and 64 bytes per subsequence, the mixed and ragged batches, and every such frame cut in half.
The barrier / LDS choreography of the real kernel (staging of the tables, the rotating round flags, the wave-level scan) is OUTSIDE this
check: it runs on the GPU only.

    python tools/jpegdec_host_check.py [--cxx /opt/rocm/lib/llvm/bin/clang++]
"""
import argparse
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'coarse-fine-networks_amd', 'csrc')
sys.path.insert(0, os.path.join(ROOT, 'coarse-fine-networks_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import jpeg_cases as jc  # noqa: E402
from cfn_hip import jpegdec  # noqa: E402

SHIM = r'''
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <cstdint>
#include <algorithm>
#include <vector>
#define __global__
#define __device__
#define __forceinline__ inline
#define __constant__
#define __launch_bounds__(x)
#define __shared__
static inline void __syncthreads() {}
struct D3 { unsigned x, y, z; };
static D3 threadIdx, blockIdx;
static inline int atomicOr(int* p, int v) { int o = *p; *p |= v; return o; }
using std::min; using std::max;
static inline int cfn_uni(int v) { return v; }
static inline int __shfl_up(int v, int, int) { return v; }
static inline int __shfl(int v, int, int) { return v; }
#include "jpegdec.h"
#include "kern.inc"
unsigned long jp_sync_lds[1];
#include <fstream>
#include <iterator>

static long al(long v) { return (v + 255) & ~255L; }

// the rounds, the scan and the write pass of jpeg_entropy_sync_kernel as a serial loop over jpeg_sub_decode
static int sync_taken = 0;                 // frames the sync mode took
static void sync_rows(const JpegArgs& a, int S, int max_subs) {
    for (int r = 0; r < a.rows; ++r) {
        const JpegRow f = jpeg_row(a, r);
        JpegGrid g = {};
        if (f.ok) g = jpeg_grid(a, f.clip);
        const int n = jpeg_sync_subs(f, g, S, max_subs);
        if (n == 0) continue;
        a.owner[f.lane0] = -1;
        ++sync_taken;
        const int* huff = a.tables + (long)JP_SET_WORDS * f.set + JP_SET_HUFF;
        std::vector<unsigned long> was(n), now(n);
        std::vector<JpegSub> rec(n);
        for (int j = 0; j < n; ++j) {
            jpeg_sub_decode(a, f, g, r, huff, jpeg_sync_start(a, f, j, S), std::min((j + 1) * S, f.bytes), false, 0, 0, 0, 0, &rec[j]);
            was[j] = rec[j].exit | JP_SYNC_CHG;
        }
        for (int k = 1; k < n; ++k) {
            bool moved = false;
            for (int j = 0; j < n; ++j) {
                const unsigned long own = was[j] & ~JP_SYNC_CHG;
                if (j == 0) { now[0] = own; continue; }
                const unsigned long pe = was[j - 1], spec = jpeg_sync_start(a, f, j, S);
                const unsigned long entry = (pe & ~JP_SYNC_CHG) == JP_SYNC_INVALID ? spec : (pe & ~JP_SYNC_CHG);
                if (!(pe & JP_SYNC_CHG) || (k == 1 && entry == spec)) { now[j] = own; continue; }
                jpeg_sub_decode(a, f, g, r, huff, entry, std::min((j + 1) * S, f.bytes), false, 0, 0, 0, 0, &rec[j]);
                const bool c = rec[j].exit != own;
                now[j] = rec[j].exit | (c ? JP_SYNC_CHG : 0ul);
                moved = moved || c;
            }
            was.swap(now);
            if (!moved) break;
        }
        int first = 0, p0 = 0, p1 = 0, p2 = 0, err = 0;
        for (int j = 0; j < n; ++j) {
            const unsigned long entry = j == 0 ? 0ul : (was[j - 1] & ~JP_SYNC_CHG);
            const JpegSub c = rec[j];
            if (entry != JP_SYNC_INVALID && first >= 0 && first < g.nblocks) {
                JpegSub s;
                err |= jpeg_sub_decode(a, f, g, r, huff, entry, std::min((j + 1) * S, f.bytes), true, first, p0, p1, p2, &s);
                if (j == n - 1 && !err && first + s.blocks < g.nblocks) err = JP_ST_DATA;
            }
            first += c.blocks; p0 += c.dc0; p1 += c.dc1; p2 += c.dc2;
        }
        if (err) a.status[r] |= err;
    }
}

extern "C" int run(const unsigned char* data, const int* frames, const int* tables, const int* geom, const int* lengths, unsigned char* out,
                   int* status, long data_bytes, int rows, int sets, int N, int T, int H, int W, int lanes, int blocks_max, int S, int max_subs) {
    JpegArgs a = {};
    a.data = data; a.frames = frames; a.tables = tables; a.geom = geom; a.lengths = lengths; a.out = out; a.status = status;
    a.data_bytes = data_bytes; a.rows = rows; a.sets = sets; a.N = N; a.T = T; a.H = H; a.W = W; a.lanes = lanes; a.blocks_max = blocks_max;
    long blocks = (long)rows * blocks_max;
    std::vector<short> coef(blocks * 64, 0);
    std::vector<int> starts(lanes, 0), owner(lanes, -1), rowmap((long)N * T, -1);
    std::vector<unsigned char> samp(blocks * 64, 0xAB);
    a.coef = coef.data(); a.starts = starts.data(); a.owner = owner.data(); a.rowmap = rowmap.data(); a.samp = samp.data();
    memset(status, 0, 4 * rows);
    // scan, serially (the kernel's wave logic is not emulated here)
    for (int r = 0; r < rows; ++r) {
        JpegRow f = jpeg_row(a, r);
        bool ok = f.ok; JpegGrid g = {};
        if (ok) { g = jpeg_grid(a, f.clip); ok = g.ok && f.lanes == jpeg_intervals(g, f.ri); }
        if (!ok) { status[r] |= 1; continue; }
        rowmap[(long)f.clip * T + f.t] = r;
        for (int i = 0; i < f.lanes; ++i) owner[f.lane0 + i] = r;
        int k = 0;
        for (int p = 0; p + 2 <= f.bytes; ++p)
            if (data[f.off + p] == 0xFF && (data[f.off + p + 1] & 0xF8) == 0xD0) { ++k; if (k < f.lanes) starts[f.lane0 + k] = p + 2; }
    }
    if (S > 0) sync_rows(a, S, max_subs);
    int per_wave = std::min(64, std::max(1, lanes / 4096));
    for (unsigned b = 0; b < (unsigned)((lanes + per_wave - 1) / per_wave); ++b)
        for (unsigned t = 0; t < 64; ++t) { blockIdx.x = b; threadIdx.x = t; jpeg_entropy_kernel(a, per_wave); }
    for (unsigned b = 0; b < (unsigned)((blocks + 255) / 256); ++b)
        for (unsigned t = 0; t < 256; ++t) { blockIdx.x = b; threadIdx.x = t; jpeg_idct_kernel(a); }
    long pixels = (long)N * T * H * W;
    for (unsigned b = 0; b < (unsigned)((pixels + 1023) / 1024); ++b)
        for (unsigned t = 0; t < 256; ++t) { blockIdx.x = b; threadIdx.x = t; jpeg_colour_kernel(a); }
    return 0;
}

template <class T> static std::vector<T> rd(const char* dir, const char* name) {
    std::ifstream f(std::string(dir) + "/" + name, std::ios::binary);
    std::vector<char> b((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    std::vector<T> v(b.size() / sizeof(T)); memcpy(v.data(), b.data(), v.size() * sizeof(T)); return v;
}
int main(int argc, char** argv) {
    const char* d = argv[1];
    auto data = rd<unsigned char>(d, "data"); auto frames = rd<int>(d, "frames"); auto tables = rd<int>(d, "tables");
    auto geom = rd<int>(d, "geom"); auto lengths = rd<int>(d, "lengths"); auto dims = rd<int>(d, "dims");
    int rows = frames.size() / 8, sets = tables.size() / 3456, N = lengths.size();
    std::vector<unsigned char> out((long)N * dims[0] * dims[1] * dims[2] * 3, 0xCD);
    std::vector<int> status(rows, 77);
    run(data.data(), frames.data(), tables.data(), geom.data(), lengths.data(), out.data(), status.data(), (long)data.size(), rows, sets, N, dims[0], dims[1], dims[2], dims[3], dims[4],
        argc > 2 ? atoi(argv[2]) : 0, argc > 3 ? atoi(argv[3]) : JP_SYNC_MAX_SUBS);
    std::ofstream(std::string(d) + "/out", std::ios::binary).write((const char*)out.data(), out.size());
    std::ofstream(std::string(d) + "/taken", std::ios::binary).write((const char*)&sync_taken, 4);
    std::ofstream(std::string(d) + "/status", std::ios::binary).write((const char*)status.data(), status.size() * 4);
    return 0;
}
'''


def build(cxx, tmp):
    with open(os.path.join(CSRC, 'jpegdec.hip')) as fh:
        src = fh.read()
    src = src[:src.index('// ---- host ----')].replace('#include "cfn_common.h"', '').replace('#include "jpegdec.h"', '')
    with open(os.path.join(tmp, 'kern.inc'), 'w') as fh:
        fh.write(src)
    with open(os.path.join(tmp, 'shim.cpp'), 'w') as fh:
        fh.write(SHIM)
    exe = os.path.join(tmp, 'shim')
    subprocess.run([cxx, '-O1', '-g', '-std=c++17', '-w', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-I' + CSRC, '-I' + tmp,
                    os.path.join(tmp, 'shim.cpp'), '-o', exe], check=True)
    return exe


def run(exe, clips, d, sub_bytes=0, max_subs=jpegdec.SYNC_MAX_SUBS):
    """sub_bytes = 0: the lane-per-interval decode; otherwise the sync mode with that subsequence size"""
    os.makedirs(d, exist_ok=True)
    for k in ('data', 'frames', 'tables'):
        getattr(clips, k).numpy().tofile(os.path.join(d, k))
    clips.geom.reshape(-1, 4).numpy().tofile(os.path.join(d, 'geom'))
    clips.lengths.reshape(-1).numpy().tofile(os.path.join(d, 'lengths'))
    np.array(clips.dims, dtype=np.int32).tofile(os.path.join(d, 'dims'))
    subprocess.run([exe, d, str(sub_bytes), str(max_subs)], check=True)
    T, H, W = clips.dims[:3]
    return (torch.from_numpy(np.fromfile(os.path.join(d, 'out'), dtype=np.uint8)).view(tuple(clips.lengths.shape) + (T, H, W, 3)),
            np.fromfile(os.path.join(d, 'status'), dtype=np.int32))


def sync_checks(exe, tmp):
    """the sync entropy mode: 0 differing bytes, cut frames flagged (and only they)"""
    bad = 0
    plain = [n for n in jc.names() if jpegdec.parse(jc.jpg(n)).restart_interval == 0]
    for name in plain:
        clips = jpegdec.collate_jpeg([([[jc.jpg(name)]], torch.tensor([jc.full_box(name)]))])
        for sub in (16, 32, 64):
            out, st = run(exe, clips, os.path.join(tmp, 'one'), sub)
            diff = int((out[0, 0, 0].numpy() != jc.pixels(name)).sum())
            taken = int(np.fromfile(os.path.join(tmp, 'one', 'taken'), dtype=np.int32)[0])
            if diff or st.any() or taken != (1 if int(clips.frames[0, jpegdec.F_BYTES]) > sub else 0):
                bad += 1
                print('FAIL sync', name, sub, diff, st, taken)
            fr = clips.frames.clone()
            fr[0, jpegdec.F_BYTES] //= 2
            _, st2 = run(exe, clips._replace(frames=fr), os.path.join(tmp, 'one'), sub)
            if st2[0] == 0:
                bad += 1
                print('FAIL sync cut', name, sub, st2)
    for tag, cl in (('mixed', jc.MIXED), ('ragged', jc.RAGGED)):
        clips = jpegdec.collate_jpeg(jc.jpeg_samples(cl, jc.MIXED_BOX if cl is jc.MIXED else jc.RAGGED_BOX))
        for sub, most in ((16, jpegdec.SYNC_MAX_SUBS), (16, 4), (64, jpegdec.SYNC_MAX_SUBS)):
            out, st = run(exe, clips, os.path.join(tmp, tag), sub, most)
            ok = torch.equal(out, jc.padded(cl)) and not st.any()
            bad += 0 if ok else 1
            print('sync', tag, sub, most, 'ok' if ok else 'FAIL', st)
        for row in range(clips.frames.shape[0]):
            fr = clips.frames.clone()
            fr[row, jpegdec.F_BYTES] //= 2
            out2, st2 = run(exe, clips._replace(frames=fr), os.path.join(tmp, tag), 16)
            whole = jc.padded(cl).reshape((-1,) + tuple(out2.shape[2:]))
            got = out2.reshape(whole.shape)
            exact = all(torch.equal(got[int(c), int(t)], whole[int(c), int(t)]) for i, (c, t) in enumerate(clips.frames[:, :2].tolist()) if i != row)
            if st2[row] == 0 or any(s for i, s in enumerate(st2) if i != row) or not exact:
                bad += 1
                print('FAIL sync cut row', row, st2, exact)
    print('sync mode: %d frames without restart markers' % len(plain))
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cxx', default=os.environ.get('CXX_HOST_CHECK', '/opt/rocm/lib/llvm/bin/clang++'))
    a = ap.parse_args()
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(a.cxx, tmp)
        for name in jc.names():
            out, st = run(exe, jpegdec.collate_jpeg([([[jc.jpg(name)]], torch.tensor([jc.full_box(name)]))]), os.path.join(tmp, 'one'))
            diff = int((out[0, 0, 0].numpy() != jc.pixels(name)).sum())
            if diff or st.any():
                bad += 1
                print('FAIL', name, diff, st)
        for tag, cl, bx in (('mixed', jc.MIXED, jc.MIXED_BOX), ('ragged', jc.RAGGED, jc.RAGGED_BOX)):
            clips = jpegdec.collate_jpeg(jc.jpeg_samples(cl, bx))
            out, st = run(exe, clips, os.path.join(tmp, tag))
            ok = torch.equal(out, jc.padded(cl)) and not st.any()
            bad += 0 if ok else 1
            print(tag, 'ok' if ok else 'FAIL', st)
            for row in range(clips.frames.shape[0]):
                fr = clips.frames.clone()
                fr[row, jpegdec.F_BYTES] //= 2
                out2, st2 = run(exe, clips._replace(frames=fr), os.path.join(tmp, tag))
                others = [s for i, s in enumerate(st2) if i != row]
                if st2[row] == 0 or any(others):
                    bad += 1
                    print('FAIL cut row', row, st2)
        bad += sync_checks(exe, tmp)
    print('%d fixtures, failures: %d' % (len(jc.names()), bad))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
