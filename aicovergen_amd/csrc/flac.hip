// A finished cover as a FLAC file (RFC 9639), encoded where the mix lives.  16-bit PCM, one or two channels, a fixed block
// size; the file is "fLaC", one STREAMINFO block (MD5 left zero: "not computed") and the frames -- no seek table, no tags.
//   * flac_subframe_kernel: one workgroup per (frame, channel candidate).  Mono has one candidate, stereo four (left, right, mid, side;
//     side is a 17-bit channel).  The candidate's samples sit in LDS as int32.  Subframe candidates, in this order: CONSTANT, VERBATIM,
//     FIXED 0..4, LPC 1..8 (Welch window, float64 autocorrelation and Levinson-Durbin, 12-bit coefficients with a shift >= 0, the
//     prediction summed in 64 bits).  FIXED and LPC are one routine: a FIXED predictor is an LPC predictor with binomial coefficients
//     and shift 0.  For a predictor the residual's cost is counted EXACTLY: per finest partition (block >> 6 samples) the sum of
//     zigzag(r) >> k for k = 0..14 and the largest magnitude go to an LDS table with integer atomics; a node per (partition order,
//     partition) merges them and takes the cheapest of the 15 Rice parameters and the escape code (raw bits; only where it is
//     shorter); the cheapest partition order wins.  The subframe with the fewest bits wins, a tie goes to the earlier candidate.
//     The winner is then written: code lengths are prefix-summed over the workgroup, every lane adds its fields into zeroed LDS words
//     (fields never overlap, so an add is an or), and the words go to the (frame, candidate) slot with ordinary stores.
//   * flac_plan_kernel: one workgroup.  Per frame the stereo mode with the fewest bits (independent, left/side, side/right, mid/side;
//     a tie to the earlier), the frame's byte size, an exclusive scan into file offsets, the smallest and largest frame; writes the
//     42 header bytes and the file's size.
//   * flac_frame_kernel: one workgroup per frame.  Header with the UTF-8-like frame number and CRC-8, the two subframes joined at bit
//     granularity straight into the file at the frame's offset, zero padding, CRC-16.  CRC is linear: lane t folds bytes t, t + 256, ...
//     with x^2048, is advanced by what follows its last byte, and the lanes' remainders are xor-ed.
#include "reduce.h"

namespace aicg {

constexpr int kFlacMaxBlock = 4096;
constexpr int kFlacFine = 64;                  // finest partitions: partition order 6
constexpr int kFlacMaxPorder = 6;
constexpr int kFlacNPred = 13;                 // FIXED 0..4, LPC 1..8
constexpr int kFlacMaxLpc = 8;
constexpr int kFlacPrec = 12;                  // bits of a quantised LPC coefficient
constexpr int kFlacHeader = 42;                // "fLaC" + metadata block header + STREAMINFO
constexpr int kFlacFrameHeaderMax = 16;
constexpr unsigned kFlacCostCap = 1u << 19;    // a sample's unary length is counted up to here: beyond, the escape code is cheaper anyway
constexpr unsigned kFlacNodeCap = 1u << 24;    // a partition's cost is counted up to here: beyond, VERBATIM is cheaper anyway
constexpr long kFlacMaxSamples = (1L << 36) - 1;

__host__ __device__ inline int flac_slot_words(int block) { return (8 + block * 17 + 31) / 32 + 1; }
__host__ __device__ inline bool flac_block_ok(int block) { return block == 256 || block == 512 || block == 1024 || block == 2048 || block == 4096; }

// workspace: offsets int64 [nf], sub_bits int32 [nf][4], mode int32 [nf] (padded to 16 bytes), slots uint32 [nf][cands][slot_words]
struct FlacWs { long off_offsets, off_bits, off_mode, off_slots, bytes; };
inline FlacWs flac_ws(long nf, int channels, int block) {
    FlacWs w;
    w.off_offsets = 0;
    w.off_bits = nf * 8;
    w.off_mode = w.off_bits + nf * 16;
    w.off_slots = (w.off_mode + nf * 4 + 15) / 16 * 16;
    w.bytes = w.off_slots + nf * (channels == 2 ? 4 : 1) * (long)flac_slot_words(block) * 4 + 16;
    return w;
}

// sample-rate code of a frame header and the bytes of its tail field
__host__ __device__ inline int flac_rate_code(int sr, int* tail) {
    *tail = 0;
    switch (sr) {
        case 88200: return 1; case 176400: return 2; case 192000: return 3; case 8000: return 4; case 16000: return 5; case 22050: return 6;
        case 24000: return 7; case 32000: return 8; case 44100: return 9; case 48000: return 10; case 96000: return 11;
    }
    if (sr % 1000 == 0 && sr / 1000 < 256) { *tail = 1; return 12; }
    if (sr < 65536) { *tail = 2; return 13; }
    if (sr % 10 == 0 && sr / 10 < 65536) { *tail = 2; return 14; }
    return 0;                                   // "take it from STREAMINFO"
}
__host__ __device__ inline int flac_utf8_len(long f) { return f < 0x80 ? 1 : f < 0x800 ? 2 : f < 0x10000 ? 3 : f < 0x200000 ? 4 : f < 0x4000000 ? 5 : 6; }
__host__ __device__ inline int flac_frame_header_len(long f, int bs, int block, int sr) {
    int tail;
    flac_rate_code(sr, &tail);
    return 4 + flac_utf8_len(f) + (bs != block ? (bs <= 256 ? 1 : 2) : 0) + tail + 1;
}

// the two subframes of a stereo mode: 0 independent (L, R), 1 left/side (L, S), 2 side/right (S, R), 3 mid/side (M, S)
__device__ __forceinline__ void flac_mode_pair(int mode, int* a, int* b) {
    *a = mode == 0 || mode == 1 ? 0 : mode == 2 ? 3 : 2;
    *b = mode == 0 || mode == 2 ? 1 : 3;
}

__global__ void __launch_bounds__(256) flac_subframe_kernel(const short* __restrict__ pcm, long n, int ch, int block, int slot_words,
                                                            int* __restrict__ sub_bits, unsigned* __restrict__ slots) {
    __shared__ int s[kFlacMaxBlock];
    __shared__ unsigned bitbuf[(8 + kFlacMaxBlock * 17 + 31) / 32 + 1];
    __shared__ unsigned T[kFlacFine * 16];          // [fine partition][k = 0..14 sums, 15 = largest magnitude]
    __shared__ int pred_order[kFlacNPred], pred_shift[kFlacNPred], pred_coef[kFlacNPred][kFlacMaxLpc];
    __shared__ unsigned node_bits[2 * kFlacFine];
    __shared__ int node_param[2 * kFlacFine];       // 0..14 Rice, 16 + raw bits for the escape code
    __shared__ int best[3];                         // bits, candidate in list order, partition order
    __shared__ int flags[2];                        // not constant; a residual beyond 24 bits
    __shared__ double acs[4][kFlacMaxLpc + 1];
    __shared__ double lev[3 * (kFlacMaxLpc + 1)];  // Levinson-Durbin's R, a and the next a (one thread; LDS keeps them out of private memory)
    __shared__ unsigned scan_sh[4];

    const int t = threadIdx.x, cand = blockIdx.y;
    const long f = blockIdx.x, start = f * (long)block;
    const int bs = (int)lmin((long)block, n - start);
    const int bps = cand == 3 ? 17 : 16;
    if (bs <= 0) return;

    for (int i = t; i < bs; i += 256) {
        const long idx = (start + i) * ch;
        const int l = pcm[idx], r = ch == 2 ? pcm[idx + 1] : l;
        s[i] = cand == 0 ? l : cand == 1 ? r : cand == 2 ? (l + r) >> 1 : l - r;
    }
    if (t == 0) { flags[0] = 0; flags[1] = 0; best[0] = 8 + bps; best[1] = 0; best[2] = 0; }
    __syncthreads();

    // CONSTANT?  and the windowed autocorrelation at lags 0..8
    {
        const double c = 0.5 * (bs - 1), d = 1.0 / (0.5 * (bs + 1));
        double ac[kFlacMaxLpc + 1];
#pragma unroll
        for (int l = 0; l <= kFlacMaxLpc; ++l) ac[l] = 0.0;
        bool same = true;
        const int s0 = s[0];
        for (int i = t; i < bs; i += 256) {
            same = same && s[i] == s0;
            const double u = (i - c) * d, x = (1.0 - u * u) * s[i];
#pragma unroll
            for (int l = 0; l <= kFlacMaxLpc; ++l)
                if (i >= l) {
                    const double v = (i - l - c) * d;
                    ac[l] += x * ((1.0 - v * v) * s[i - l]);
                }
        }
        if (!same) flags[0] = 1;
#pragma unroll
        for (int l = 0; l <= kFlacMaxLpc; ++l) {
            const double v = wave_sum(ac[l]);
            if ((t & 63) == 0) acs[t >> 6][l] = v;
        }
    }
    __syncthreads();

    if (t == 0) {
        for (int p = 0; p < 5; ++p) {               // FIXED order p: coefficient j = (-1)^j C(p, j + 1)
            pred_order[p] = p;
            pred_shift[p] = 0;
            int c = 1;
            for (int j = 0; j < kFlacMaxLpc; ++j) {
                c = j < p ? c * (p - j) / (j + 1) : 0;
                pred_coef[p][j] = (j & 1) ? -c : c;
            }
        }
        double* R = lev, *a = lev + (kFlacMaxLpc + 1), *b = lev + 2 * (kFlacMaxLpc + 1);
        for (int l = 0; l <= kFlacMaxLpc; ++l) R[l] = ((acs[0][l] + acs[1][l]) + acs[2][l]) + acs[3][l];
        double E = R[0];
        bool alive = E > 0.0;
        for (int m = 1; m <= kFlacMaxLpc; ++m) {
            const int p = 4 + m;
            pred_order[p] = -1;
            pred_shift[p] = 0;
            for (int j = 0; j < kFlacMaxLpc; ++j) pred_coef[p][j] = 0;
            if (!alive) continue;
            double k = R[m];
            for (int j = 1; j < m; ++j) k -= a[j] * R[m - j];
            k /= E;
            if (!(k > -1.0 && k < 1.0)) { alive = false; continue; }
            for (int j = 1; j < m; ++j) b[j] = a[j] - k * a[m - j];
            for (int j = 1; j < m; ++j) a[j] = b[j];
            a[m] = k;
            E *= 1.0 - k * k;
            if (!(E > 0.0)) alive = false;       // this order is still a predictor; no further one
            double cmax = 0.0;
            for (int j = 1; j <= m; ++j) cmax = fmax(cmax, fabs(a[j]));
            if (!(cmax > 0.0 && cmax < 1e6)) continue;
            int sh = 15;
            while (sh > 0 && cmax * (double)(1 << sh) > 2047.0) --sh;
            double e = 0.0;
            for (int j = 1; j <= m; ++j) {
                const double v = a[j] * (double)(1 << sh) + e;
                long q = (long)floor(v + 0.5);
                q = lmax(-2048, lmin(2047, q));
                e = v - (double)q;
                pred_coef[p][j - 1] = (int)q;
            }
            pred_order[p] = m;
            pred_shift[p] = sh;
        }
    }
    __syncthreads();

    int pmax = 0;
    while (pmax < kFlacMaxPorder && ((bs >> pmax) & 1) == 0) ++pmax;
    const int P = bs >> pmax;                        // samples of a finest partition
    const int spt = (bs + 255) / 256, i0 = t * spt, i1 = imin(bs, i0 + spt);

    auto residual = [&](int i, int order, int shift, const int* coef) -> long long {
        long long pr = 0;
#pragma unroll
        for (int j = 0; j < kFlacMaxLpc; ++j)
            if (j < order) pr += (long long)coef[j] * s[i - 1 - j];
        return (long long)s[i] - (pr >> shift);
    };
    auto zigzag = [&](long long r) -> unsigned {
        const unsigned long long z = ((unsigned long long)r << 1) ^ (unsigned long long)(r >> 63);
        return z >= (1ull << 25) ? (1u << 25) - 1u : (unsigned)z;
    };

    // exact cost of predictor p at every partition order it may take; thread 0 keeps the best (bits, candidate, partition order)
    auto eval = [&](int p) {
        const int order = pred_order[p], shift = pred_shift[p];
        int coef[kFlacMaxLpc];
#pragma unroll
        for (int j = 0; j < kFlacMaxLpc; ++j) coef[j] = pred_coef[p][j];
        for (int q = t; q < kFlacFine * 16; q += 256) T[q] = 0u;
        if (t == 0) flags[1] = 0;
        __syncthreads();
        {
            unsigned acc[15], mx = 0u;
            int cur = -1;
            bool bad = false;
            for (int i = imax(i0, order); i < i1; ++i) {
                const int part = i / P;
                if (part != cur) {
                    if (cur >= 0) {
#pragma unroll
                        for (int k = 0; k < 15; ++k) atomicAdd(&T[cur * 16 + k], acc[k]);
                        atomicMax(&T[cur * 16 + 15], mx);
                    }
                    cur = part;
                    mx = 0u;
#pragma unroll
                    for (int k = 0; k < 15; ++k) acc[k] = 0u;
                }
                const long long r = residual(i, order, shift, coef);
                const unsigned long long mag = (unsigned long long)(r ^ (r >> 63));
                bad = bad || mag >= (1ull << 24);
                mx = mx > (unsigned)lmin((long)mag, (1L << 24)) ? mx : (unsigned)lmin((long)mag, (1L << 24));
                const unsigned z = zigzag(r);
#pragma unroll
                for (int k = 0; k < 15; ++k) {
                    const unsigned u = z >> k;
                    acc[k] += u < kFlacCostCap ? u : kFlacCostCap;
                }
            }
            if (cur >= 0) {
#pragma unroll
                for (int k = 0; k < 15; ++k) atomicAdd(&T[cur * 16 + k], acc[k]);
                atomicMax(&T[cur * 16 + 15], mx);
            }
            if (bad) flags[1] = 1;
        }
        __syncthreads();
        int pc = 0;                                   // the largest partition order: 2^pc divides bs and a partition holds more than `order`
        while (pc < pmax && (bs >> (pc + 1)) > order) ++pc;
        if (t < (2 << pc) - 1) {
            const int po = 31 - __builtin_clz((unsigned)(t + 1)), q = t + 1 - (1 << po), span = 1 << (pmax - po);
            const unsigned cnt = (unsigned)((bs >> po) - (q == 0 ? order : 0));
            unsigned long long sum[15];
            unsigned mx = 0u;
#pragma unroll
            for (int k = 0; k < 15; ++k) sum[k] = 0ull;
            for (int g = q * span; g < (q + 1) * span; ++g) {
#pragma unroll
                for (int k = 0; k < 15; ++k) sum[k] += T[g * 16 + k];
                mx = mx > T[g * 16 + 15] ? mx : T[g * 16 + 15];
            }
            unsigned long long bc = ~0ull;
            int bk = 0;
#pragma unroll
            for (int k = 0; k < 15; ++k) {
                const unsigned long long c = 4ull + sum[k] + (unsigned long long)(k + 1) * cnt;
                if (c < bc) { bc = c; bk = k; }
            }
            const int nb = mx == 0u ? 1 : 33 - __builtin_clz(mx);
            const unsigned long long esc = 9ull + (unsigned long long)nb * cnt;
            if (esc < bc) { bc = esc; bk = 16 + nb; }
            node_bits[t] = bc < kFlacNodeCap ? (unsigned)bc : kFlacNodeCap;
            node_param[t] = bk;
        }
        __syncthreads();
        if (t == 0 && flags[1] == 0) {
            const int head = 8 + order * bps + (p >= 5 ? 9 + order * kFlacPrec : 0) + 6;
            for (int po = 0; po <= pc; ++po) {
                long tot = head;
                for (int q = 0; q < (1 << po); ++q) tot += node_bits[(1 << po) - 1 + q];
                if (tot < (long)best[0]) { best[0] = (int)tot; best[1] = 2 + p; best[2] = po; }
            }
        }
    };

    if (flags[0] != 0) {                             // (uniform: LDS value read after a barrier)
        if (t == 0) { best[0] = 8 + bs * bps; best[1] = 1; best[2] = 0; }
        for (int p = 0; p < kFlacNPred; ++p) {
            if (pred_order[p] < 0 || pred_order[p] >= bs) continue;
            eval(p);
        }
    }
    __syncthreads();
    const int win = best[1], porder = best[2];
    if (win >= 2) {
        __syncthreads();
        eval(win - 2);                               // leaves the winner's Rice parameters in node_param
        __syncthreads();
    }

    const int words = slot_words;
    for (int w = t; w < words; w += 256) bitbuf[w] = 0u;
    __syncthreads();
    auto put = [&](long pos, unsigned val, int nbits) {   // nbits <= 32, val < 2^nbits; MSB first
        if (nbits <= 0) return;
        const int w = (int)(pos >> 5), o = (int)(pos & 31);
        if (o + nbits <= 32) {
            if (w < words) atomicAdd(&bitbuf[w], val << (32 - o - nbits));
        } else {
            const int lo = o + nbits - 32;
            if (w < words) atomicAdd(&bitbuf[w], val >> lo);
            if (w + 1 < words) atomicAdd(&bitbuf[w + 1], val << (32 - lo));
        }
    };
    const unsigned smask = (1u << bps) - 1u;
    unsigned total = 0u;
    if (win == 0) {
        if (t == 0) put(8, (unsigned)s[0] & smask, bps);
        total = 8 + bps;
    } else if (win == 1) {
        if (t == 0) put(0, 1u << 1, 8);
        for (int i = t; i < bs; i += 256) put(8 + (long)i * bps, (unsigned)s[i] & smask, bps);
        total = 8 + bs * bps;
    } else {
        const int p = win - 2, order = pred_order[p], shift = pred_shift[p];
        int coef[kFlacMaxLpc];
#pragma unroll
        for (int j = 0; j < kFlacMaxLpc; ++j) coef[j] = pred_coef[p][j];
        if (t == 0) put(0, (p < 5 ? (8u | (unsigned)order) : (32u | (unsigned)(order - 1))) << 1, 8);
        if (t < order) put(8 + (long)t * bps, (unsigned)s[t] & smask, bps);
        long pos = 8 + (long)order * bps;
        if (p >= 5) {
            if (t == 0) { put(pos, kFlacPrec - 1, 4); put(pos + 4, (unsigned)shift, 5); }
            if (t < order) put(pos + 9 + (long)t * kFlacPrec, (unsigned)pred_coef[p][t] & 0xfffu, kFlacPrec);
            pos += 9 + order * kFlacPrec;
        }
        if (t == 0) put(pos + 2, (unsigned)porder, 4);        // (the two method bits in front are 00: 4-bit parameters)
        pos += 6;
        const int Pp = bs >> porder, node0 = (1 << porder) - 1;
        unsigned len = 0u;
        for (int i = imax(i0, order); i < i1; ++i) {
            const int q = i / Pp, prm = node_param[node0 + q];
            if (i == (q == 0 ? order : q * Pp)) len += prm >= 16 ? 9u : 4u;
            len += prm >= 16 ? (unsigned)(prm - 16) : (zigzag(residual(i, order, shift, coef)) >> prm) + 1u + (unsigned)prm;
        }
        unsigned inc = len;
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned v = __shfl_up(inc, (unsigned)o, 64);
            if ((t & 63) >= o) inc += v;
        }
        if ((t & 63) == 63) scan_sh[t >> 6] = inc;
        __syncthreads();
        unsigned base = 0u;
        for (int w = 0; w < (t >> 6); ++w) base += scan_sh[w];
        total = (unsigned)pos + scan_sh[0] + scan_sh[1] + scan_sh[2] + scan_sh[3];
        long at = pos + base + inc - len;
        for (int i = imax(i0, order); i < i1; ++i) {
            const int q = i / Pp, prm = node_param[node0 + q];
            const long long r = residual(i, order, shift, coef);
            if (i == (q == 0 ? order : q * Pp)) {
                if (prm >= 16) { put(at, 15u, 4); put(at + 4, (unsigned)(prm - 16), 5); at += 9; }
                else { put(at, (unsigned)prm, 4); at += 4; }
            }
            if (prm >= 16) {
                const int nb = prm - 16;
                put(at, (unsigned)r & ((1u << nb) - 1u), nb);
                at += nb;
            } else {
                const unsigned z = zigzag(r);
                at += z >> prm;
                put(at, (1u << prm) | (z & ((1u << prm) - 1u)), prm + 1);
                at += prm + 1;
            }
        }
    }
    __syncthreads();
    unsigned* slot = slots + (f * gridDim.y + cand) * (long)slot_words;
    const int used = imin(words, (int)((total + 31u) >> 5));
    for (int w = t; w < used; w += 256) slot[w] = bitbuf[w];
    if (t == 0) sub_bits[f * 4 + cand] = (int)total;
}

__global__ void __launch_bounds__(256) flac_plan_kernel(const int* __restrict__ sub_bits, long nf, long n, int ch, int block, int sr,
                                                        long long* __restrict__ offsets, int* __restrict__ mode_out,
                                                        unsigned char* __restrict__ out, long long* __restrict__ n_bytes) {
    __shared__ unsigned scan_sh[4];
    __shared__ unsigned ext[2];                     // largest frame, ~smallest frame
    const int t = threadIdx.x;
    if (t == 0) { ext[0] = 0u; ext[1] = 0u; }
    long long run = kFlacHeader;
    unsigned big = 0u, small = 0xffffffffu;
    for (long base = 0; base < nf; base += 256) {
        const long f = base + t;
        unsigned size = 0u;
        if (f < nf) {
            const int bs = (int)lmin((long)block, n - f * block);
            const int* b = sub_bits + f * 4;
            int bits = b[0], mode = 0;
            if (ch == 2) {
                bits = b[0] + b[1];
                if (b[0] + b[3] < bits) { bits = b[0] + b[3]; mode = 1; }
                if (b[3] + b[1] < bits) { bits = b[3] + b[1]; mode = 2; }
                if (b[2] + b[3] < bits) { bits = b[2] + b[3]; mode = 3; }
            }
            mode_out[f] = mode;
            size = (unsigned)(flac_frame_header_len(f, bs, block, sr) + (bits + 7) / 8 + 2);
            big = size > big ? size : big;
            small = size < small ? size : small;
        }
        unsigned inc = size;
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned v = __shfl_up(inc, (unsigned)o, 64);
            if ((t & 63) >= o) inc += v;
        }
        __syncthreads();                             // the previous round's reads of scan_sh are over
        if ((t & 63) == 63) scan_sh[t >> 6] = inc;
        __syncthreads();
        unsigned before = 0u;
        for (int w = 0; w < (t >> 6); ++w) before += scan_sh[w];
        if (f < nf) offsets[f] = run + before + inc - size;
        run += (long long)scan_sh[0] + scan_sh[1] + scan_sh[2] + scan_sh[3];
    }
    if (nf > 0) {
        atomicMax(&ext[0], big);
        atomicMax(&ext[1], ~small);
    }
    __syncthreads();
    if (t == 0) {
        const unsigned mn = nf > 0 ? ~ext[1] : 0u, mx = ext[0];
        const unsigned long long ns = (unsigned long long)n;
        const unsigned char sig[8] = {'f', 'L', 'a', 'C', 0x80, 0, 0, 34};      // one STREAMINFO block of 34 bytes, marked last
#pragma unroll
        for (int i = 0; i < 8; ++i) out[i] = sig[i];
        out[8] = out[10] = (unsigned char)(block >> 8);
        out[9] = out[11] = (unsigned char)block;
        out[12] = (unsigned char)(mn >> 16); out[13] = (unsigned char)(mn >> 8); out[14] = (unsigned char)mn;
        out[15] = (unsigned char)(mx >> 16); out[16] = (unsigned char)(mx >> 8); out[17] = (unsigned char)mx;
        out[18] = (unsigned char)(sr >> 12);
        out[19] = (unsigned char)(sr >> 4);
        out[20] = (unsigned char)(((sr & 15) << 4) | ((ch - 1) << 1));         // 16 bits a sample: 15 = 0b01111, its top bit here
        out[21] = (unsigned char)(0xf0 | ((ns >> 32) & 15));
        out[22] = (unsigned char)(ns >> 24); out[23] = (unsigned char)(ns >> 16); out[24] = (unsigned char)(ns >> 8); out[25] = (unsigned char)ns;
        for (int i = 26; i < kFlacHeader; ++i) out[i] = (unsigned char)0;       // MD5: zero = not computed
        n_bytes[0] = run;
    }
}

// CRC-16 (x^16 + x^15 + x^2 + 1, initial value 0) as arithmetic in GF(2)[x] / P
__device__ __forceinline__ unsigned crc16_mul(unsigned a, unsigned b) {
    unsigned r = 0u;
    for (int i = 15; i >= 0; --i) {
        r = ((r << 1) ^ ((r & 0x8000u) ? 0x8005u : 0u)) & 0xffffu;
        if ((b >> i) & 1u) r ^= a;
    }
    return r;
}
__device__ __forceinline__ unsigned crc16_xpow8(long nbytes) {      // x^(8 nbytes) mod P
    unsigned r = 1u, b = 0x100u;
    for (; nbytes > 0; nbytes >>= 1) {
        if (nbytes & 1) r = crc16_mul(r, b);
        b = crc16_mul(b, b);
    }
    return r;
}
__device__ __forceinline__ unsigned crc16_byte(unsigned byte) {     // byte x^16 mod P
    unsigned v = byte << 8;
    for (int i = 0; i < 8; ++i) v = ((v << 1) ^ ((v & 0x8000u) ? 0x8005u : 0u)) & 0xffffu;
    return v;
}

// eight bits from bit `pos` of a subframe of nbits (MSB-first words); zero past its end
__device__ __forceinline__ unsigned flac_read8(const unsigned* __restrict__ w, long nbits, long pos) {
    if (pos >= nbits) return 0u;
    const long wi = pos >> 5;
    const int o = (int)(pos & 31);
    const unsigned long long two = ((unsigned long long)w[wi] << 32) | (o > 24 && (wi + 1) * 32 < nbits ? w[wi + 1] : 0u);
    unsigned b = (unsigned)(two >> (56 - o)) & 0xffu;
    const long rem = nbits - pos;
    if (rem < 8) b &= 0xffu << (8 - rem);
    return b & 0xffu;
}

__global__ void __launch_bounds__(256) flac_frame_kernel(const int* __restrict__ sub_bits, const unsigned* __restrict__ slots,
                                                         const long long* __restrict__ offsets, const int* __restrict__ mode_in, long n,
                                                         int ch, int block, int sr, int slot_words, unsigned char* __restrict__ out,
                                                         long long capacity) {
    __shared__ unsigned char hdr[kFlacFrameHeaderMax];
    __shared__ int hdr_len;
    __shared__ unsigned crc_sh[4];
    const int t = threadIdx.x;
    const long f = blockIdx.x;
    const int bs = (int)lmin((long)block, n - f * block), mode = mode_in[f];
    if (t == 0) {
        int tail, k = 0;
        const int rate = flac_rate_code(sr, &tail);
        const int bcode = bs != block ? (bs <= 256 ? 6 : 7) : block == 256 ? 8 : block == 512 ? 9 : block == 1024 ? 10 : block == 2048 ? 11 : 12;
        hdr[k++] = 0xff;
        hdr[k++] = 0xf8;                            // sync, fixed block size
        hdr[k++] = (unsigned char)((bcode << 4) | rate);
        hdr[k++] = (unsigned char)(((ch == 1 ? 0 : mode == 0 ? 1 : 7 + mode) << 4) | (4 << 1));       // 16 bits a sample
        const int nb = flac_utf8_len(f);
        if (nb == 1) hdr[k++] = (unsigned char)f;
        else {
            hdr[k++] = (unsigned char)((0xff00 >> nb) | (f >> (6 * (nb - 1))));
            for (int j = nb - 2; j >= 0; --j) hdr[k++] = (unsigned char)(0x80 | ((f >> (6 * j)) & 0x3f));
        }
        if (bcode == 6) hdr[k++] = (unsigned char)(bs - 1);
        if (bcode == 7) { hdr[k++] = (unsigned char)((bs - 1) >> 8); hdr[k++] = (unsigned char)(bs - 1); }
        const int rv = rate == 12 ? sr / 1000 : rate == 14 ? sr / 10 : sr;
        if (tail == 2) hdr[k++] = (unsigned char)(rv >> 8);
        if (tail >= 1) hdr[k++] = (unsigned char)rv;
        unsigned c = 0u;
        for (int j = 0; j < k; ++j) {
            c ^= hdr[j];
            for (int i = 0; i < 8; ++i) c = ((c << 1) ^ ((c & 0x80u) ? 0x07u : 0u)) & 0xffu;
        }
        hdr[k++] = (unsigned char)c;
        hdr_len = k;
    }
    __syncthreads();
    int ia = 0, ib = 0;
    flac_mode_pair(mode, &ia, &ib);
    const int cands = ch == 2 ? 4 : 1;
    const long bits_a = sub_bits[f * 4 + ia], bits_b = ch == 2 ? sub_bits[f * 4 + ib] : 0;
    const unsigned* A = slots + (f * cands + ia) * (long)slot_words;
    const unsigned* B = slots + (f * cands + (ch == 2 ? ib : 0)) * (long)slot_words;
    const int hl = hdr_len;
    const long N = hl + (bits_a + bits_b + 7) / 8, off = offsets[f];
    if (off + N + 2 > capacity) return;             // cannot happen for a capacity from aicg_flac_geometry
    const unsigned x256 = crc16_xpow8(256);
    unsigned acc = 0u;
    long last = -1;
    for (long j = t; j < N; j += 256) {
        unsigned byte;
        if (j < hl) byte = hdr[j];
        else {
            const long v = (j - hl) * 8;
            if (v >= bits_a) byte = flac_read8(B, bits_b, v - bits_a);
            else {
                byte = flac_read8(A, bits_a, v);
                if (v + 8 > bits_a) byte |= flac_read8(B, bits_b, 0) >> (bits_a - v);
            }
        }
        out[off + j] = (unsigned char)byte;
        acc = crc16_mul(acc, x256) ^ crc16_byte(byte);
        last = j;
    }
    if (last >= 0) acc = crc16_mul(acc, crc16_xpow8(N - 1 - last));
    for (int o = 32; o > 0; o >>= 1) acc ^= __shfl_xor(acc, o, 64);
    if ((t & 63) == 0) crc_sh[t >> 6] = acc;
    __syncthreads();
    if (t == 0) {
        const unsigned c = crc_sh[0] ^ crc_sh[1] ^ crc_sh[2] ^ crc_sh[3];
        out[off + N] = (unsigned char)(c >> 8);
        out[off + N + 1] = (unsigned char)c;
    }
}

static int flac_shape(const char* who, int64_t n, int channels, int sample_rate, int block) {
    if (channels < 1 || channels > 2) return fail(AICG_E_SHAPE, "%s: %d channels (1 or 2 are encoded)", who, channels);
    if (!flac_block_ok(block)) return fail(AICG_E_ARG, "%s: block size %d (256, 512, 1024, 2048 or 4096)", who, block);
    if (sample_rate < 1 || sample_rate >= (1 << 20)) return fail(AICG_E_ARG, "%s: sample rate %d", who, sample_rate);
    if (n < 0 || n > kFlacMaxSamples || ldiv_up((long)n, block) > 0x7fffffffL)
        return fail(AICG_E_SHAPE, "%s: %lld samples a channel", who, (long long)n);
    return AICG_OK;
}

}  // namespace aicg

using namespace aicg;

extern "C" int aicg_flac_geometry(int64_t n, int channels, int sample_rate, int block, int64_t* geom) {
    if (int rc = flac_shape("aicg_flac_geometry", n, channels, sample_rate, block)) return rc;
    if (!geom) return fail(AICG_E_ARG, "aicg_flac_geometry: null pointer");
    const long nf = ldiv_up((long)n, block);
    geom[0] = nf;
    geom[1] = flac_ws(nf, channels, block).bytes;
    geom[2] = kFlacHeader + nf * (kFlacFrameHeaderMax + 2 + (long)channels * flac_slot_words(block) * 4);
    geom[3] = flac_slot_words(block);
    return AICG_OK;
}

extern "C" int aicg_flac_encode(const void* pcm, int64_t n, int channels, int sample_rate, int block, void* workspace, void* out,
                                int64_t capacity, int64_t* n_bytes, void* stream) {
    if (int rc = flac_shape("aicg_flac_encode", n, channels, sample_rate, block)) return rc;
    const long nf = ldiv_up((long)n, block);
    if (!out || !n_bytes || !workspace || (n > 0 && !pcm)) return fail(AICG_E_ARG, "aicg_flac_encode: null pointer");
    if (capacity < kFlacHeader + nf * (kFlacFrameHeaderMax + 2 + (long)channels * flac_slot_words(block) * 4))
        return fail(AICG_E_ARG, "aicg_flac_encode: capacity %lld below aicg_flac_geometry's", (long long)capacity);
    hipStream_t st = (hipStream_t)stream;
    const FlacWs w = flac_ws(nf, channels, block);
    char* ws = (char*)workspace;
    long long* offsets = (long long*)(ws + w.off_offsets);
    int* bits = (int*)(ws + w.off_bits);
    int* mode = (int*)(ws + w.off_mode);
    unsigned* slots = (unsigned*)(ws + w.off_slots);
    const int sw = flac_slot_words(block);
    if (nf > 0)
        hipLaunchKernelGGL(flac_subframe_kernel, dim3((unsigned)nf, channels == 2 ? 4 : 1), dim3(256), 0, st, (const short*)pcm, (long)n,
                           channels, block, sw, bits, slots);
    hipLaunchKernelGGL(flac_plan_kernel, dim3(1), dim3(256), 0, st, (const int*)bits, nf, (long)n, channels, block, sample_rate, offsets,
                       mode, (unsigned char*)out, (long long*)n_bytes);
    if (nf > 0)
        hipLaunchKernelGGL(flac_frame_kernel, dim3((unsigned)nf), dim3(256), 0, st, (const int*)bits, (const unsigned*)slots,
                           (const long long*)offsets, (const int*)mode, (long)n, channels, block, sample_rate, sw, (unsigned char*)out,
                           (long long)capacity);
    return check_launch("flac_subframe_kernel");
}
