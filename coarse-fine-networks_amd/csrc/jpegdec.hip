// Baseline JPEG frames decoded on the GPU, bit for bit like PIL with libjpeg (cfn_hip/jpegdec.py: the host side, the batch type and the
// numpy statement of the same arithmetic).  Replaces the reference's per-frame host decode, Image.open(f).convert('RGB') in pil_loader /
// video_loader of charades_fine.py and charades_coarse_fineFEAT.py.  Four kernels behind one entry point (capi.hip cfn_jpeg_decode_u8),
// all on the caller's stream, working in a caller-provided workspace:
//
//   scan     one WAVE per frame: checks the frame's record against the batch, enters the frame into the (clip, t) -> row map and the
//            decoder lanes' owner list, and finds the RSTn markers of its segment (FF D0..D7 never occurs inside entropy-coded data), whose
//            ordinals give every restart interval its first byte
//   entropy  one LANE per (frame, restart interval): Huffman decode (9-bit lookahead table, then maxcode / valoff by length), DC
//            prediction, run / size symbols with EOB and ZRL -> quantised int16 coefficients in natural order, [frame][component]
//            [block row][block column][64], zero-filled by the same call
//   idct     one lane per 8 x 8 block: dequantise, libjpeg's jidctint ("islow") in int32 -> planar 8-bit Y, Cb, Cr
//   colour   one lane per 4 output pixels (12 bytes): "fancy" triangle upsampling for h2v2 / h2v1, the fixed-point YCbCr -> RGB of
//            jdcolor, gray replication; writes EVERY byte of the RawU8Clips frames (N, Tmax, Hmax, Wmax, 3): the picture in the top-left
//            corner, zero bytes outside h x w and in frames nothing was decoded into
//
// A second entry point (cfn_jpeg_decode_u8_sync) puts a fifth kernel between scan and entropy:
//
//   entropy, sync   one WORKGROUP per frame without restart markers, one lane per subsequence of S raw bytes: speculative decodes in rounds
//            until no exit state changes, a scan of block counts and DC sums, one write pass (see the section in front of the host code);
//            the frames it takes are struck from the owner list, every other frame is left to the entropy kernel above
//
// Everything the kernels index with is DATA (records, offsets, lengths, tables, geometry): every loop has a bound that does not depend on
// the bit stream (<= 16 bits per code, <= 63 AC symbols per block, block and MCU counts from the checked geometry), every read of `data`
// is clamped to the frame's own segment, every table index is masked, every workspace index is derived from the checked geometry.  A
// frame that fails a check, runs out of data or meets an invalid code sets bits in its status word and stops; it never reads or writes
// outside its own ranges.
#include "cfn_common.h"
#include "jpegdec.h"

#define JP_COLS 8                  // ints per frame record: clip, t, offset, bytes, table set, restart interval, first lane, lanes
#define JP_LOOK 9
#define JP_HT_MAXCODE 512
#define JP_HT_VALOFF 544
#define JP_HT_VAL 576
#define JP_HT_WORDS 832
#define JP_SET_HUFF 128
#define JP_SET_WORDS (128 + 4 * JP_HT_WORDS)
#define JP_ST_ROW 1
#define JP_ST_DATA 2
#define JP_ST_CODE 4

typedef unsigned __attribute__((ext_vector_type(4))) jp_u4;
typedef unsigned __attribute__((ext_vector_type(2))) jp_u2;

static __constant__ unsigned char jp_zigzag[64] = {
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// the block grid of a clip, from geom (h, w, sampling code, components); ok = inside the batch's extents
struct JpegGrid { int h, w, ncomp, hs, vs, mx, my, bw0, nb0, nbc, nblocks; bool ok; };

__device__ __forceinline__ JpegGrid jpeg_grid(const JpegArgs& a, int clip) {
    const int* g = a.geom + 4L * clip;
    JpegGrid q;
    q.h = g[0]; q.w = g[1]; q.ncomp = g[3];
    const int s = g[2];
    q.hs = q.ncomp == 1 ? 1 : (s >> 4);
    q.vs = q.ncomp == 1 ? 1 : (s & 15);
    q.ok = q.h >= 1 && q.h <= a.H && q.w >= 1 && q.w <= a.W && (q.ncomp == 1 || q.ncomp == 3) &&
           (q.ncomp == 1 || s == 0x11 || s == 0x21 || s == 0x22);
    if (!q.ok) { q.hs = q.vs = 1; q.h = q.w = 1; q.ncomp = 1; }
    q.mx = (q.w + 8 * q.hs - 1) / (8 * q.hs);
    q.my = (q.h + 8 * q.vs - 1) / (8 * q.vs);
    q.bw0 = q.mx * q.hs;
    q.nb0 = q.bw0 * q.my * q.vs;
    q.nbc = q.ncomp == 3 ? q.mx * q.my : 0;
    q.nblocks = q.nb0 + 2 * q.nbc;
    q.ok = q.ok && q.nblocks <= a.blocks_max;
    return q;
}

struct JpegRow { int clip, t, off, bytes, set, ri, lane0, lanes; bool ok; };

// a frame's record, checked against the batch; every kernel derives its indices from the checked copy
__device__ __forceinline__ JpegRow jpeg_row(const JpegArgs& a, int r) {
    const int* f = a.frames + (long)JP_COLS * r;
    JpegRow q;
    q.clip = f[0]; q.t = f[1]; q.off = f[2]; q.bytes = f[3]; q.set = f[4]; q.ri = f[5]; q.lane0 = f[6]; q.lanes = f[7];
    q.ok = q.clip >= 0 && q.clip < a.N && q.t >= 0 && q.t < a.T && q.off >= 0 && (q.off & 3) == 0 && q.bytes >= 0 &&
           (long)q.off + (((long)q.bytes + 3) & ~3L) <= a.data_bytes && q.set >= 0 && q.set < a.sets && q.ri >= 0 && q.lane0 >= 0 && q.lanes >= 1 &&
           (long)q.lane0 + q.lanes <= a.lanes;
    if (q.ok) q.ok = q.t < a.lengths[q.clip];
    return q;
}

__device__ __forceinline__ int jpeg_intervals(const JpegGrid& g, int ri) {
    const int nmcu = g.mx * g.my;
    return ri > 0 ? (nmcu + ri - 1) / ri : 1;
}

// ---- scan ----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void jpeg_scan_kernel(const JpegArgs a) {
    const int lane = threadIdx.x & 63;
    const int r = cfn_uni((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    if (r >= a.rows) return;
    const JpegRow f = jpeg_row(a, r);
    JpegGrid g = {};
    bool ok = f.ok;
    if (ok) { g = jpeg_grid(a, f.clip); ok = g.ok && f.lanes == jpeg_intervals(g, f.ri); }
    if (!ok) {
        if (lane == 0) atomicOr(a.status + r, JP_ST_ROW);
        return;
    }
    if (lane == 0) a.rowmap[(long)f.clip * a.T + f.t] = r;
    for (int i = lane; i < f.lanes; i += 64) a.owner[f.lane0 + i] = r;
    if (f.lanes == 1) return;
    // RSTn markers in stream order: the k-th one ends interval k and the byte behind it starts interval k + 1
    const unsigned char* p = a.data + f.off;
    int base = 0;
    const int words = (f.bytes + 3) >> 2;                    // (the segment starts on a 4-byte boundary and is followed by >= 8 zero bytes)
    for (int w0 = 0; w0 < words; w0 += 64) {
        const int wi = w0 + lane;
        unsigned lo = 0, hi = 0;
        if (wi < words) {
            lo = *reinterpret_cast<const unsigned*>(p + 4L * wi);
            if (wi + 1 < words) hi = *reinterpret_cast<const unsigned*>(p + 4L * wi + 4);
        }
        const unsigned long v = ((unsigned long)hi << 32) | lo;
        int pos[4], n = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned b0 = (unsigned)(v >> (8 * j)) & 255u, b1 = (unsigned)(v >> (8 * j + 8)) & 255u;
            const bool m = b0 == 0xFFu && (b1 & 0xF8u) == 0xD0u && 4 * wi + j + 2 <= f.bytes;
            pos[j] = m ? 4 * wi + j + 2 : -1;
            n += m ? 1 : 0;
        }
        int incl = n;                                        // inclusive prefix sum of the lanes' counts
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int u = __shfl_up(incl, o, 64);
            if (lane >= o) incl += u;
        }
        int k = base + incl - n;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (pos[j] >= 0) {
                ++k;
                if (k < f.lanes) a.starts[f.lane0 + k] = pos[j];
            }
        base += __shfl(incl, 63, 64);
    }
}

// ---- entropy ---------------------------------------------------------------------------------------------------------------------------
struct JpegBits {
    const unsigned char* p; int pos, end; unsigned long acc; int cnt, pad; bool stop;
    // at least 57 valid bits behind this; behind the end of the interval (its end, or a marker) zero bits are fed and counted
    __device__ __forceinline__ void refill() {
#pragma unroll 1
        for (int i = 0; i < 8; ++i) {
            if (cnt > 56) break;
            unsigned b = 0;
            bool real = false;
            if (!stop && pos < end) {
                b = p[pos];
                if (b == 0xFFu) {
                    const unsigned b2 = pos + 1 < end ? p[pos + 1] : 0xFFu;
                    if (b2 == 0u) { pos += 2; real = true; } else { stop = true; b = 0; }
                } else { pos += 1; real = true; }
            }
            pad += real ? 0 : 1;
            acc = (acc << 8) | b;
            cnt += 8;
        }
    }
    __device__ __forceinline__ unsigned peek16() const { return (unsigned)(acc >> (cnt - 16)) & 0xFFFFu; }
    __device__ __forceinline__ int receive(int s) {          // s <= 15 bits, sign-extended as libjpeg's HUFF_EXTEND
        const int v = (int)((acc >> (cnt - s)) & ((1u << s) - 1u));
        cnt -= s;
        return (s == 0 || v >= (1 << (s - 1))) ? v : v - (1 << s) + 1;
    }
    // one Huffman symbol; -1 for a code that is in no table
    __device__ __forceinline__ int symbol(const int* ht) {
        refill();
        const unsigned pk = peek16();
        const int e = ht[pk >> (16 - JP_LOOK)];
        int len = e >> 8, sym = e & 255;
        if (len == 0) {
            sym = -1;
#pragma unroll 1
            for (int l = JP_LOOK + 1; l <= 16; ++l) {
                const int code = (int)(pk >> (16 - l));
                if (code <= ht[JP_HT_MAXCODE + l]) { sym = ht[JP_HT_VAL + ((ht[JP_HT_VALOFF + l] + code) & 255)] & 255; len = l; break; }
            }
            if (sym < 0) return -1;
        }
        cnt -= len & 31;
        return sym;
    }
};

__global__ __launch_bounds__(64) void jpeg_entropy_kernel(const JpegArgs a, int per_wave) {
    if ((int)threadIdx.x >= per_wave) return;
    const long L = (long)blockIdx.x * per_wave + threadIdx.x;
    if (L >= a.lanes) return;
    const int r = a.owner[L];
    if (r < 0 || r >= a.rows) return;
    const JpegRow f = jpeg_row(a, r);
    if (!f.ok) return;
    const JpegGrid g = jpeg_grid(a, f.clip);
    const int idx = (int)(L - f.lane0);
    if (!g.ok || idx < 0 || idx >= f.lanes || f.lanes != jpeg_intervals(g, f.ri)) return;
    int start = 0;
    if (idx > 0) {
        start = a.starts[L];
        if (start <= 0 || start > f.bytes) { atomicOr(a.status + r, JP_ST_DATA); return; }       // the marker in front of this interval is missing
    }
    const int nmcu = g.mx * g.my;
    const int k0 = f.ri > 0 ? idx * f.ri : 0;
    const int k1 = f.ri > 0 ? min(k0 + f.ri, nmcu) : nmcu;
    const int* set = a.tables + (long)JP_SET_WORDS * f.set;
    short* coef = a.coef + (long)r * a.blocks_max * 64;
    JpegBits br;
    br.p = a.data + f.off; br.pos = start; br.end = f.bytes; br.acc = 0; br.cnt = 0; br.pad = 0; br.stop = false;
    int pred[3] = {0, 0, 0};
    int err = 0;
#pragma unroll 1
    for (int k = k0; k < k1 && !err; ++k) {
        const int my = k / g.mx, mx = k - my * g.mx;
#pragma unroll 1
        for (int c = 0; c < g.ncomp && !err; ++c) {
            const int hs = c ? 1 : g.hs, vs = c ? 1 : g.vs, slot = c ? 1 : 0;
            const int* dc = set + JP_SET_HUFF + slot * JP_HT_WORDS;
            const int* ac = set + JP_SET_HUFF + (2 + slot) * JP_HT_WORDS;
            const int pbase = c == 0 ? 0 : (c == 1 ? g.nb0 : g.nb0 + g.nbc);
            const int bw = g.mx * hs;
#pragma unroll 1
            for (int bi = 0; bi < hs * vs && !err; ++bi) {
                const int by = bi / hs, bx = bi - by * hs;
                short* blk = coef + ((long)pbase + (long)(my * vs + by) * bw + (mx * hs + bx)) * 64;
                int s = br.symbol(dc);
                if (s < 0) { err = JP_ST_CODE; break; }
                pred[c] += br.receive(s & 15);
                blk[0] = (short)pred[c];
                int i = 1;
#pragma unroll 1
                for (int it = 0; it < 63 && i < 64; ++it) {
                    s = br.symbol(ac);
                    if (s < 0) { err = JP_ST_CODE; break; }
                    const int run = s >> 4, sz = s & 15;
                    if (sz == 0) {
                        if (run != 15) break;                // EOB
                        i += 16;                             // ZRL
                        continue;
                    }
                    i += run;
                    if (i > 63) { err = JP_ST_CODE; break; }
                    blk[jp_zigzag[i & 63]] = (short)br.receive(sz);
                    ++i;
                }
            }
        }
    }
    if (!err && br.pad * 8 > br.cnt) err = JP_ST_DATA;       // bits were taken from behind the interval's end
    if (err) atomicOr(a.status + r, err);
}

// ---- dequantise + inverse DCT ------------------------------------------------------------------------------------------------------------
// one 1-D pass of jidctint: 8 inputs -> 8 outputs, descaled by `shift` (libjpeg computes in `long`; int32 holds every intermediate for
// coefficients a real encoder emits)
__device__ __forceinline__ void jpeg_idct8(const int i0, const int i1, const int i2, const int i3, const int i4, const int i5, const int i6,
                                           const int i7, const int shift, int* o) {
    int z1 = (i2 + i6) * 4433;
    const int t2 = z1 - i6 * 15137, t3 = z1 + i2 * 6270;
    const int t0 = (int)((unsigned)(i0 + i4) << 13), t1 = (int)((unsigned)(i0 - i4) << 13);
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    int a0 = i7, a1 = i5, a2 = i3, a3 = i1;
    z1 = a0 + a3;
    int z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3;
    const int z5 = (z3 + z4) * 9633;
    a0 *= 2446; a1 *= 16819; a2 *= 25172; a3 *= 12299;
    z1 *= -7373; z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    a0 += z1 + z3; a1 += z2 + z4; a2 += z2 + z3; a3 += z1 + z4;
    const int rnd = 1 << (shift - 1);
    o[0] = (t10 + a3 + rnd) >> shift; o[7] = (t10 - a3 + rnd) >> shift;
    o[1] = (t11 + a2 + rnd) >> shift; o[6] = (t11 - a2 + rnd) >> shift;
    o[2] = (t12 + a1 + rnd) >> shift; o[5] = (t12 - a1 + rnd) >> shift;
    o[3] = (t13 + a0 + rnd) >> shift; o[4] = (t13 - a0 + rnd) >> shift;
}

__global__ __launch_bounds__(256) void jpeg_idct_kernel(const JpegArgs a) {
    const long gid = (long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= (long)a.rows * a.blocks_max) return;
    const int r = (int)(gid / a.blocks_max), b = (int)(gid - (long)r * a.blocks_max);
    const JpegRow f = jpeg_row(a, r);
    if (!f.ok) return;
    const JpegGrid g = jpeg_grid(a, f.clip);
    if (!g.ok || b >= g.nblocks) return;
    const int c = b < g.nb0 ? 0 : (b < g.nb0 + g.nbc ? 1 : 2);
    const int pbase = c == 0 ? 0 : (c == 1 ? g.nb0 : g.nb0 + g.nbc);
    const int bw = c == 0 ? g.bw0 : g.mx;
    const int by = (b - pbase) / bw, bx = (b - pbase) - by * bw;
    const int* qt = a.tables + (long)JP_SET_WORDS * f.set + (c ? 64 : 0);
    const jp_u4* src = reinterpret_cast<const jp_u4*>(a.coef + ((long)r * a.blocks_max + b) * 64);
    int ws[64];
#pragma unroll
    for (int row = 0; row < 8; ++row) {
        const jp_u4 v = src[row];
        const unsigned u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            ws[row * 8 + 2 * j] = (int)(short)(u[j] & 0xFFFFu) * qt[row * 8 + 2 * j];
            ws[row * 8 + 2 * j + 1] = (int)(short)(u[j] >> 16) * qt[row * 8 + 2 * j + 1];
        }
    }
#pragma unroll
    for (int col = 0; col < 8; ++col) {                      // pass 1: down the columns
        int o[8];
        jpeg_idct8(ws[col], ws[8 + col], ws[16 + col], ws[24 + col], ws[32 + col], ws[40 + col], ws[48 + col], ws[56 + col], 11, o);
#pragma unroll
        for (int j = 0; j < 8; ++j) ws[8 * j + col] = o[j];
    }
    unsigned char* dst = a.samp + ((long)r * a.blocks_max + pbase) * 64 + ((long)by * 8 * bw + bx) * 8;
#pragma unroll
    for (int row = 0; row < 8; ++row) {                      // pass 2: along the rows
        int o[8];
        jpeg_idct8(ws[8 * row], ws[8 * row + 1], ws[8 * row + 2], ws[8 * row + 3], ws[8 * row + 4], ws[8 * row + 5], ws[8 * row + 6],
                   ws[8 * row + 7], 18, o);
        unsigned w[2] = {0u, 0u};
#pragma unroll
        for (int j = 0; j < 8; ++j) w[j >> 2] |= (unsigned)min(max(o[j] + 128, 0), 255) << (8 * (j & 3));
        *reinterpret_cast<jp_u2*>(dst + (long)row * bw * 8) = jp_u2{w[0], w[1]};
    }
}

// ---- upsample + colour ---------------------------------------------------------------------------------------------------------------------
// the chroma sample of pixel (y, x): libjpeg's h2v2 / h2v1 "fancy" (triangle) upsampling over the dh x dw REAL samples of the plane
__device__ __forceinline__ int jpeg_chroma(const unsigned char* p, int stride, const JpegGrid& g, int y, int x) {
    if (g.hs == 1) return p[(long)y * stride + x];
    const int dw = (g.w + 1) >> 1, c = x >> 1;
    const int cn = (x & 1) ? min(c + 1, dw - 1) : max(c - 1, 0);
    if (g.vs == 1) {
        const unsigned char* q = p + (long)y * stride;
        return (3 * q[c] + q[cn] + 1 + (x & 1)) >> 2;
    }
    const int dh = (g.h + 1) >> 1, rr = y >> 1;
    const int ro = (y & 1) ? min(rr + 1, dh - 1) : max(rr - 1, 0);
    const unsigned char* q0 = p + (long)rr * stride;
    const unsigned char* q1 = p + (long)ro * stride;
    const int cs = 3 * q0[c] + q1[c], csn = 3 * q0[cn] + q1[cn];
    return (3 * cs + csn + 8 - (x & 1)) >> 4;
}

__device__ __forceinline__ unsigned jpeg_clamp8(int v) { return (unsigned)min(max(v, 0), 255); }

__global__ __launch_bounds__(256) void jpeg_colour_kernel(const JpegArgs a) {
    const long pixels = (long)a.N * a.T * a.H * a.W;
    const long p0 = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (p0 >= pixels) return;
    long rest = p0;
    int x = (int)(rest % a.W); rest /= a.W;
    int y = (int)(rest % a.H); rest /= a.H;
    long z = rest;                                           // clip * Tmax + t
    unsigned char px[12];
    long zc = -1;
    int row = -1;
    JpegGrid g = {};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        unsigned R = 0, G = 0, B = 0;
        if (p0 + j < pixels) {
            if (z != zc) {
                zc = z;
                row = a.rowmap[z];
                if (row >= a.rows) row = -1;
                if (row >= 0) { g = jpeg_grid(a, (int)(z / a.T)); if (!g.ok) row = -1; }
            }
            if (row >= 0 && y < g.h && x < g.w) {
                const unsigned char* s = a.samp + (long)row * a.blocks_max * 64;
                const int Y = s[(long)y * g.bw0 * 8 + x];
                if (g.ncomp == 1) {
                    R = G = B = (unsigned)Y;
                } else {
                    const int cstride = g.mx * 8;
                    const int cb = jpeg_chroma(s + (long)g.nb0 * 64, cstride, g, y, x) - 128;
                    const int cr = jpeg_chroma(s + (long)(g.nb0 + g.nbc) * 64, cstride, g, y, x) - 128;
                    R = jpeg_clamp8(Y + ((91881 * cr + 32768) >> 16));
                    G = jpeg_clamp8(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
                    B = jpeg_clamp8(Y + ((116130 * cb + 32768) >> 16));
                }
            }
        }
        px[3 * j] = (unsigned char)R; px[3 * j + 1] = (unsigned char)G; px[3 * j + 2] = (unsigned char)B;
        if (++x == a.W) { x = 0; if (++y == a.H) { y = 0; ++z; } }
    }
    unsigned char* dst = a.out + 3 * p0;                     // 12 bytes per lane on a 4-byte boundary (the base is checked on the host)
    if (p0 + 4 <= pixels) {
#pragma unroll
        for (int j = 0; j < 3; ++j)
            reinterpret_cast<unsigned*>(dst)[j] = (unsigned)px[4 * j] | ((unsigned)px[4 * j + 1] << 8) | ((unsigned)px[4 * j + 2] << 16) |
                                                  ((unsigned)px[4 * j + 3] << 24);
    } else {
        const int n = (int)(pixels - p0) * 3;
#pragma unroll
        for (int j = 0; j < 12; ++j)
            if (j < n) dst[j] = px[j];
    }
}

// ---- entropy, 'sync' mode: parallel inside a frame without restart markers -------------------------------------------------------------------
// Huffman-coded data self-synchronises (Weissenberger & Schmidt, "Accelerating JPEG Decompression on GPUs"); the rounds, and why n of
// them always reach the true states, are stated in plain Python by cfn_hip/jpegdec.py decode_coefficients_sync.  One workgroup per frame
// row.  A frame is taken when its record has restart interval 0 (one decoder lane), more than `S` bytes and at most `max_subs`
// subsequences of S raw bytes; the workgroup then clears the frame's entry in the owner list, so that jpeg_entropy_kernel, launched
// behind this kernel, passes over it and decodes every other frame as before.
//
// A decoder state is one 64-bit word: raw byte index << 32 | bit << 12 | unit of the MCU << 8 | zigzag index; bit 15 says "changed in
// this round" and takes no part in comparisons.  The byte behind a data byte FF is skipped whatever it is and bytes behind the segment's
// end read as 0, so a subsequence's decode is a pure function of its entry state.
#define JP_SYNC_INVALID 0xFFFFFFFF00000000ul
#define JP_SYNC_CHG 0x8000ul

__device__ __forceinline__ unsigned long jpeg_sync_pack(int p, int b, int u, int zz) {
    return ((unsigned long)(unsigned)p << 32) | (unsigned long)(unsigned)((b << 12) | (u << 8) | zz);
}

// the subsequences of a frame the sync mode takes, 0 for every other frame
__device__ __forceinline__ int jpeg_sync_subs(const JpegRow& f, const JpegGrid& g, int S, int max_subs) {
    if (!f.ok || !g.ok || f.ri != 0 || f.lanes != 1 || f.bytes <= S) return 0;
    const long n = ((long)f.bytes + S - 1) / S;
    return n <= max_subs ? (int)n : 0;
}

// the speculative entry of subsequence j < n: its first byte, one on when that is the stuffed 00 of an FF 00 pair; u = zz = 0
__device__ __forceinline__ unsigned long jpeg_sync_start(const JpegArgs& a, const JpegRow& f, int j, int S) {
    if (j <= 0) return 0ul;
    const int p = j * S;
    return jpeg_sync_pack(p + (a.data[(long)f.off + p - 1] == 0xFFu ? 1 : 0), 0, 0, 0);
}

// the bit reader of the sync mode: JpegBits' buffer, plus one flag per buffered byte (was it FF, i.e. two raw bytes) from which the raw
// position of the next bit is recovered.  Raw bytes come from aligned dword loads (the segment starts on a 4-byte boundary, the row
// check says so), in address order whatever the bytes hold, so the next dword is always on its way while the current one is used.
struct JpegSyncBits {
    const unsigned* w; int pos, end; unsigned q, nxt; int qn, wi; unsigned long acc; int cnt; unsigned ffm;
    // dword i of the segment, bytes at or behind `end` zeroed; nothing is read at or behind end rounded up to 4
    __device__ __forceinline__ unsigned dword(int i) const {
        const int rest = end - 4 * i;
        if (i < 0 || rest <= 0) return 0u;
        const unsigned v = w[i];
        return rest >= 4 ? v : (v & ((1u << (8 * rest)) - 1u));
    }
    __device__ __forceinline__ void start(const unsigned char* seg, int p0, int bytes) {      // 0 <= p0 <= bytes
        w = reinterpret_cast<const unsigned*>(seg); pos = p0; end = bytes; acc = 0; cnt = 0; ffm = 0;
        wi = p0 >> 2;
        q = dword(wi) >> (8 * (p0 & 3)); qn = 4 - (p0 & 3);
        nxt = dword(wi + 1);
        wi += 2;
    }
    __device__ __forceinline__ unsigned byte() {             // raw byte `pos`; 0 behind the end
        if (qn == 0) { q = nxt; qn = 4; nxt = dword(wi); ++wi; }
        const unsigned b = q & 255u;
        q >>= 8; --qn; ++pos;
        return b;
    }
    __device__ __forceinline__ void refill() {               // at least 57 valid bits behind this
#pragma unroll 1
        for (int i = 0; i < 8; ++i) {
            if (cnt > 56) break;
            const unsigned b = byte();
            const unsigned ff = b == 0xFFu ? 1u : 0u;
            if (ff) byte();                                  // the byte behind FF is skipped whatever it is
            acc = (acc << 8) | b;
            ffm = (ffm << 1) | ff;
            cnt += 8;
        }
    }
    // the raw byte that holds the next bit, and the bit's index in it (cnt >= 1: call behind refill)
    __device__ __forceinline__ int head_byte() const {
        const int h = (cnt - 1) >> 3;
        return pos - (h + 1) - __builtin_popcount(ffm & ((2u << h) - 1u));
    }
    __device__ __forceinline__ int head_bit() const { return (8 - (cnt & 7)) & 7; }
    __device__ __forceinline__ unsigned peek16() const { return (unsigned)(acc >> (cnt - 16)) & 0xFFFFu; }
    __device__ __forceinline__ int receive(int s) {
        const int v = (int)((acc >> (cnt - s)) & ((1u << s) - 1u));
        cnt -= s;
        return (s == 0 || v >= (1 << (s - 1))) ? v : v - (1 << s) + 1;
    }
    __device__ __forceinline__ int symbol(const int* ht) {   // as JpegBits::symbol, the caller refills
        const unsigned pk = peek16();
        const int e = ht[pk >> (16 - JP_LOOK)];
        int len = e >> 8, sym = e & 255;
        if (len == 0) {
            sym = -1;
#pragma unroll 1
            for (int l = JP_LOOK + 1; l <= 16; ++l) {
                const int code = (int)(pk >> (16 - l));
                if (code <= ht[JP_HT_MAXCODE + l]) { sym = ht[JP_HT_VAL + ((ht[JP_HT_VALOFF + l] + code) & 255)] & 255; len = l; break; }
            }
            if (sym < 0) return -1;
        }
        cnt -= len & 31;
        return sym;
    }
};

// what a lane keeps per subsequence: the exit state, the blocks it completed, the sum of its DC differences per component
struct JpegSub { unsigned long exit; int blocks, dc0, dc1, dc2; };

// block `k` of the frame in scan order (MCU by MCU, luma units row by row, then Cb, Cr) -> its 64 coefficients; k < g.nblocks
__device__ __forceinline__ short* jpeg_scan_block(short* coef, const JpegGrid& g, int k) {
    const int ny = g.hs * g.vs, bpm = ny + (g.ncomp == 3 ? 2 : 0);
    const int m = k / bpm, u = k - m * bpm, my = m / g.mx, mx = m - my * g.mx;
    int idx;
    if (u < ny) {
        const int by = u / g.hs, bx = u - by * g.hs;
        idx = (my * g.vs + by) * g.bw0 + mx * g.hs + bx;
    } else {
        idx = (u == ny ? g.nb0 : g.nb0 + g.nbc) + my * g.mx + mx;
    }
    return coef + (long)idx * 64;
}

// One subsequence of frame `f` (row r): decode from `entry` up to the first symbol whose first bit lies at or behind raw byte `limit`
// (<= f.bytes).  `huff`: the frame's four Huffman tables (DC0, DC1, AC0, AC1).  write = false: nothing is stored and no status is set;
// an invalid code or a coefficient index beyond 63 gives the exit JP_SYNC_INVALID.  write = true: the lane continues block `first` of
// the scan (at the entry's zigzag index) with the predictors pred0..2, writes absolute DC values and AC coefficients in natural order,
// stops behind the frame's last block and returns the status bits of what it met.
__device__ __forceinline__ int jpeg_sub_decode(const JpegArgs& a, const JpegRow& f, const JpegGrid& g, int r, const int* huff, unsigned long entry,
                                               int limit, bool write, int first, int pred0, int pred1, int pred2, JpegSub* out) {
    const int ny = g.hs * g.vs, bpm = ny + (g.ncomp == 3 ? 2 : 0);
    short* coef = a.coef + (long)r * a.blocks_max * 64;
    int u = (int)(entry >> 8) & 15, zz = (int)entry & 63, bidx = first;
    if (write) u = bidx % bpm;
    if (u >= bpm) u = 0;
    int p0 = (int)(entry >> 32);
    if (p0 < 0 || p0 > limit) p0 = limit;
    const int budget = 8 * (limit - p0) + 64;                // every symbol takes a bit or more
    JpegSyncBits br;
    br.start(a.data + f.off, p0, f.bytes);
    br.refill();
    br.cnt -= (int)(entry >> 12) & 7;
    int blocks = 0, dc0 = 0, dc1 = 0, dc2 = 0, err = 0;
    short* blk = (write && bidx < g.nblocks) ? jpeg_scan_block(coef, g, bidx) : nullptr;
#pragma unroll 1
    for (int it = 0; it < budget; ++it) {
        br.refill();
        if ((br.pos >= limit && br.head_byte() >= limit) || (write && bidx >= g.nblocks)) break;      // (the head never lies behind pos)
        const int c = u < ny ? 0 : u - ny + 1, slot = c ? 1 : 0;
        if (zz == 0) {
            const int s = br.symbol(huff + slot * JP_HT_WORDS);
            if (s < 0) { err = JP_ST_CODE; break; }
            const int d = br.receive(s & 15);
            if (c == 0) { dc0 += d; pred0 += d; } else if (c == 1) { dc1 += d; pred1 += d; } else { dc2 += d; pred2 += d; }
            if (write) blk[0] = (short)(c == 0 ? pred0 : (c == 1 ? pred1 : pred2));
            zz = 1;
            continue;
        }
        const int s = br.symbol(huff + (2 + slot) * JP_HT_WORDS);
        if (s < 0) { err = JP_ST_CODE; break; }
        const int run = s >> 4, sz = s & 15;
        if (sz == 0) {
            zz = run == 15 ? zz + 16 : 64;                   // ZRL, EOB
        } else {
            zz += run;
            if (zz > 63) { err = JP_ST_CODE; break; }
            const int v = br.receive(sz);
            if (write) blk[jp_zigzag[zz & 63]] = (short)v;
            ++zz;
        }
        if (zz >= 64) {
            zz = 0;
            u = u + 1 == bpm ? 0 : u + 1;
            ++blocks; ++bidx;
            if (write && bidx < g.nblocks) blk = jpeg_scan_block(coef, g, bidx);
        }
    }
    br.refill();
    const int hp = br.head_byte(), hb = br.head_bit();
    if (write && !err && (hp > f.bytes || (hp == f.bytes && hb > 0))) err = JP_ST_DATA;       // bits were taken from behind the segment's end
    out->exit = err == JP_ST_CODE ? JP_SYNC_INVALID : jpeg_sync_pack(hp, hb, u, zz);
    out->blocks = blocks; out->dc0 = dc0; out->dc1 = dc1; out->dc2 = dc2;
    return write ? err : 0;
}

// LDS: the four Huffman tables of the frame (13,312 bytes), three round flags, and per subsequence two exit states (this round's and the
// last one's) and the four counts: 32 bytes each, dynamic, sized for max_subs <= JP_SYNC_MAX_SUBS (1536: 48 KiB, 62,480 bytes in all,
// inside the 64 KiB a launch gets without asking for more)
__global__ __launch_bounds__(JP_SYNC_THREADS) void jpeg_entropy_sync_kernel(const JpegArgs a, int S, int max_subs) {
    extern __shared__ unsigned long jp_sync_lds[];
    __shared__ int huff[4 * JP_HT_WORDS];
    __shared__ int any[4];
    const int tid = (int)threadIdx.x, r = (int)blockIdx.x;
    // the same words are read by every lane, so the workgroup leaves as a whole, in front of its first barrier
    if (r >= a.rows || S < 16 || max_subs < 1 || max_subs > JP_SYNC_MAX_SUBS) return;
    const JpegRow f = jpeg_row(a, r);
    JpegGrid g = {};
    if (f.ok) g = jpeg_grid(a, f.clip);
    const int n = jpeg_sync_subs(f, g, S, max_subs);
    if (n == 0) return;
    unsigned long* ex0 = jp_sync_lds;
    unsigned long* ex1 = jp_sync_lds + max_subs;
    int* rec = reinterpret_cast<int*>(jp_sync_lds + 2L * max_subs);
    if (tid == 0) a.owner[f.lane0] = -1;                     // jpeg_entropy_kernel passes over this frame
    const int* set = a.tables + (long)JP_SET_WORDS * f.set + JP_SET_HUFF;
    for (int i = tid; i < 4 * JP_HT_WORDS; i += JP_SYNC_THREADS) huff[i] = set[i];
    if (tid < 3) any[tid] = 0;
    __syncthreads();
    // round 0: every subsequence from its speculative start, subsequence 0 from the true state
    for (int j = tid; j < n; j += JP_SYNC_THREADS) {
        JpegSub s;
        jpeg_sub_decode(a, f, g, r, huff, jpeg_sync_start(a, f, j, S), min((j + 1) * S, f.bytes), false, 0, 0, 0, 0, &s);
        ex0[j] = s.exit | JP_SYNC_CHG;
        rec[4 * j] = s.blocks; rec[4 * j + 1] = s.dc0; rec[4 * j + 2] = s.dc1; rec[4 * j + 3] = s.dc2;
    }
    __syncthreads();
    // round k: from the predecessor's exit of round k - 1, where that is not the entry used last.  The trip count (n) and the decision to
    // stop (a flag in LDS, read behind the barrier; three flags in rotation, so that the reset never meets a reader) are uniform.
    int k = 1;
    for (; k < n; ++k) {
        const unsigned long* was = (k & 1) ? ex0 : ex1;
        unsigned long* now = (k & 1) ? ex1 : ex0;
        bool moved = false;
        for (int j = tid; j < n; j += JP_SYNC_THREADS) {
            const unsigned long own = was[j] & ~JP_SYNC_CHG;
            if (j == 0) { now[0] = own; continue; }
            const unsigned long pe = was[j - 1], spec = jpeg_sync_start(a, f, j, S);
            const unsigned long entry = (pe & ~JP_SYNC_CHG) == JP_SYNC_INVALID ? spec : (pe & ~JP_SYNC_CHG);
            if (!(pe & JP_SYNC_CHG) || (k == 1 && entry == spec)) { now[j] = own; continue; }
            JpegSub s;
            jpeg_sub_decode(a, f, g, r, huff, entry, min((j + 1) * S, f.bytes), false, 0, 0, 0, 0, &s);
            const bool c = s.exit != own;
            now[j] = s.exit | (c ? JP_SYNC_CHG : 0ul);
            rec[4 * j] = s.blocks; rec[4 * j + 1] = s.dc0; rec[4 * j + 2] = s.dc1; rec[4 * j + 3] = s.dc2;
            moved = moved || c;
        }
        if (moved) any[k % 3] = 1;
        if (tid == 0) any[(k + 1) % 3] = 0;
        __syncthreads();
        if (!any[k % 3]) break;
    }
    const unsigned long* fin = ((k < n ? k : n - 1) & 1) ? ex1 : ex0;
    // exclusive scan of the four counts over the subsequences, by the first wave: first block and entry predictors of every subsequence
    if (tid < 64) {
        int carry[4] = {0, 0, 0, 0};
        for (int base = 0; base < n; base += 64) {
            const int j = base + tid;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int v = j < n ? rec[4 * j + q] : 0;
                int incl = v;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const int t = __shfl_up(incl, o, 64);
                    if (tid >= o) incl += t;
                }
                if (j < n) rec[4 * j + q] = carry[q] + incl - v;
                carry[q] += __shfl(incl, 63, 64);
            }
        }
    }
    __syncthreads();
    // the write pass, from the true entries
    int err = 0;
    for (int j = tid; j < n; j += JP_SYNC_THREADS) {
        const unsigned long entry = j == 0 ? 0ul : (fin[j - 1] & ~JP_SYNC_CHG);
        const int first = rec[4 * j];
        if (entry == JP_SYNC_INVALID || first < 0 || first >= g.nblocks) continue;
        JpegSub s;
        err |= jpeg_sub_decode(a, f, g, r, huff, entry, min((j + 1) * S, f.bytes), true, first, rec[4 * j + 1], rec[4 * j + 2], rec[4 * j + 3], &s);
        if (j == n - 1 && !err && first + s.blocks < g.nblocks) err = JP_ST_DATA;              // the segment ended in front of the last block
    }
    if (err) atomicOr(a.status + r, err);
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------
static long jp_align(long v) { return (v + 255) & ~255L; }

// workspace: [coefficients int16 | interval starts]  zero-filled,  [lane owners | (clip, t) -> row]  filled with -1,  [8-bit samples]
void jpeg_workspace_layout(int rows, long slots, int lanes, int blocks_max, JpegLayout* l) {
    const long blocks = (long)rows * blocks_max;
    l->coef = 0;
    l->starts = jp_align(blocks * 128);
    l->owner = jp_align(l->starts + 4L * lanes);
    l->rowmap = l->owner + jp_align(4L * lanes);
    l->samp = jp_align(l->rowmap + 4L * slots);
    l->total = jp_align(l->samp + blocks * 64);
}

// sub_bytes = 0: the lane-per-interval decode alone (cfn_jpeg_decode_u8).  Otherwise the sync kernel runs between the scan and the
// lane-per-interval kernel, which then finds the frames it took struck from the owner list.
static int jpeg_decode_launch_mode(JpegArgs a, void* ws, void* stream, int sub_bytes, int max_subs, const char* who) {
    hipStream_t st = (hipStream_t)stream;
    JpegLayout l;
    jpeg_workspace_layout(a.rows, (long)a.N * a.T, a.lanes, a.blocks_max, &l);
    char* w = (char*)ws;
    a.coef = (short*)(w + l.coef); a.starts = (int*)(w + l.starts); a.owner = (int*)(w + l.owner); a.rowmap = (int*)(w + l.rowmap);
    a.samp = (unsigned char*)(w + l.samp);
    const long pixels = (long)a.N * a.T * a.H * a.W, blocks = (long)a.rows * a.blocks_max;
    const long cgrid = (pixels + 1023) / 1024, igrid = (blocks + 255) / 256;
    CFN_REQUIRE(cgrid < (1L << 31) && igrid < (1L << 31), "%s: too many pixels or blocks for one grid", who);
    CfnProfScope prof(CFN_K_ELEMWISE, st, (double)pixels * 3.0 + (double)a.data_bytes + (double)blocks * 384.0);
    if (hipMemsetAsync(w + l.coef, 0, (size_t)(l.owner - l.coef), st) != hipSuccess ||
        hipMemsetAsync(w + l.owner, 0xFF, (size_t)(l.samp - l.owner), st) != hipSuccess ||
        hipMemsetAsync(a.status, 0, 4 * (size_t)a.rows, st) != hipSuccess)
        return cfn_fail(CFN_ERR_LAUNCH, "%s: hipMemsetAsync failed: %s", who, hipGetErrorString(hipGetLastError()));
    hipLaunchKernelGGL(jpeg_scan_kernel, dim3((unsigned)((a.rows + 3) / 4)), dim3(256), 0, st, a);
    if (sub_bytes > 0)
        hipLaunchKernelGGL(jpeg_entropy_sync_kernel, dim3((unsigned)a.rows), dim3(JP_SYNC_THREADS), (size_t)max_subs * JP_SYNC_SUB_LDS, st, a, sub_bytes,
                           max_subs);
    // one lane per restart interval: a wave is only filled once there are lanes for ~4 waves on each of the 1024 SIMDs
    const int per_wave = min(64, max(1, a.lanes / 4096));
    hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((unsigned)((a.lanes + per_wave - 1) / per_wave)), dim3(64), 0, st, a, per_wave);
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)igrid), dim3(256), 0, st, a);
    hipLaunchKernelGGL(jpeg_colour_kernel, dim3((unsigned)cgrid), dim3(256), 0, st, a);
    return cfn_check_launch(who);
}

int jpeg_decode_launch(JpegArgs a, void* ws, void* stream) { return jpeg_decode_launch_mode(a, ws, stream, 0, 0, "cfn_jpeg_decode_u8"); }

int jpeg_decode_sync_launch(JpegArgs a, void* ws, void* stream, int sub_bytes, int max_subs) {
    return jpeg_decode_launch_mode(a, ws, stream, sub_bytes, max_subs, "cfn_jpeg_decode_u8_sync");
}
