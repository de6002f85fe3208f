"""Files built against the decoder's parallel entropy decode (vali_amd/csrc/jpeg_decode.hip: k_jd_unstuff, k_jd_sync,
k_jd_seams, k_jd_write), for tests/test_jpeg_hostile_host.py on the CPU and tests/test_gpu_jpeg_hostile.py on the GPU.
Pictures synchronise within a few subsequences; these streams are chosen so that they do not, or so that their
blocks, segments and code words fall on the boundaries the kernels cut the stream at.

Sim restates the synchronisation in plain Python from the kernel's header comment and the rules of decode_run<false>
(an invalid code consumes 16 bits as symbol 0, a run past 63 ends the block, ZRL is capped at 64).  It characterises
the inputs -- how long a guessed decode takes to meet the sequential one, how many passes k_jd_sync's loop makes, what
every seam walk of k_jd_seams covers and corrects -- and is never compared with the GPU: the reference of the GPU
tests is tests/jpeg_decode_model.py.

Every family is a list of Case(name, data, raw, pillow) as in tests/jpeg_variant_files.py.
A  never synchronising: every symbol costs 16 bits (12-bit codes plus size 4), the DC code read through the AC table
   is a valid symbol of the same cost and the other way round, so a decode that starts out of phase stays out of
   phase; in 4:2:0 the position in the MCU is part of the phase
B  blocks of 1665 bits, the longest a baseline block can be: 16-bit codes, DC size 11, AC size 10
C  restart structure: more than 1024 and 2048 segments, segments of exactly 1024 m - 8, 1024 m and 1024 m + 8 bits for
   m = 1, 2 and 256, A's stream in segments of 1.6 workgroups, and code words that start in the last bit of a full
   subsequence at every byte alignment of the segment start
D  a batch of A, B and C files between files of one subsequence, in two orders
E  an A file with one bit flipped in its last workgroup (a run past 63): corrupt

Measured by `python tests/test_jpeg_hostile_host.py` (subsequences, workgroups, seams, share of the subsequences that
are no segment start whose guessed decode does not meet the sequential one within 256 subsequences or before the
segment ends, longest run of subsequences without a block end, segments, share of samples at 0 or 255):
A  never gray 240x240                          858  4  3  93.5 %  0     1   0.0 %
     seams walk 256 (+1), 256 (+0), 90 (+1) subsequences (correction of tail); k_jd_sync passes 255, 255, 255, 89
A  never 420 160x160                           572  3  2  98.9 %  0     1   0.0 %
     seams walk 256 (+1), 60 (+1) subsequences (correction of tail); k_jd_sync passes 255, 255, 59
B  long blocks gray 136x136                    469  2  1   1.5 %  1     1  75.8 %
     seams walk 2 (-3) subsequences (correction of tail); k_jd_sync passes 98, 68
C  1089 segments gray 264x264                 1089  5  0   0.0 %  0  1089   0.0 %
C  2116 segments gray 368x368                 2116  9  0   0.0 %  0  2116   0.0 %
C  1056 segments 420 528x512                  1056  5  0   0.0 %  0  1056   0.0 %
C  segment lengths m 1 2                        11  1  0  40.0 %  0     6   0.0 %
C  segment lengths m 256                       769  4  2   0.1 %  0     3   0.0 %
     seams walk 1 (+1), 1 (-5) subsequences (correction of tail); k_jd_sync passes 2, 3, 4, 0
C  never gray, 1.6 workgroups a segment        802  4  3  93.8 %  0     2   0.0 %
     seams walk 145 (+1), 256 (+1), 34 (+1) subsequences (correction of tail); k_jd_sync passes 255, 144, 255, 33
C  last bit seed 0                              48  1  0  81.2 %  0    16   0.0 %
C  last bit seed 1                              48  1  0  84.4 %  0    16   0.0 %
C  last bit seed 2                              48  1  0  84.4 %  0    16   0.0 %
noise twin: 628 subsequences, catch-up median 9, largest 50
The noise twin is the Annex K q100 noise file of A's gray size: its guessed decodes meet the sequential one, its seam
walks cover 10 and 2 subsequences.  In the files of short segments (segment lengths m 1 2, last bit) most guessed
decodes reach the end of their segment first.  No stream can have two consecutive subsequences without a block end: a block, guessed or
exact, is at most 64 code words of 31 bits, 1984 bits, fewer than the 2048 bits of two subsequences."""
from __future__ import annotations

import functools

import numpy as np

import jpeg_decode_files as jf
import jpeg_decode_model as dm
import jpeg_stream_writer as sw
import jpeg_variant_files as vf
from jpeg_variant_files import Case

SUB_BITS = 1024          # kSubBits
GROUP = 256              # kGroup
CAP = 257                # subsequences a catch-up walk follows at most


# ---- the simulation ---------------------------------------------------------------------------------------------------------
def _lut(table):
    """(length, symbol) of the code at the top of every 16-bit word; no code: 16 bits as symbol 0"""
    length, sym = np.full(65536, 16, np.int64), np.zeros(65536, np.int64)
    for code, s in table.items():
        n = len(code)
        base = int(code, 2) << (16 - n)
        length[base:base + (1 << (16 - n))] = n
        sym[base:base + (1 << (16 - n))] = s
    return length, sym


class Sim:
    """the self-synchronising decode of one file, as the kernels run it.  A state is (p, c, k): the bit position in
    the image's unstuffed stream, the block's position in its MCU and the next zigzag index."""

    def __init__(self, data):
        info = dm.parse(data)
        mcux, mcuy, self.bpm = dm.geometry(info)
        nmcu = mcux * mcuy
        self.nseg = -(-nmcu // (info["ri"] or nmcu))
        segs = dm.segments(info["data"], self.nseg)
        assert segs is not None
        hv = 1 if info["nc"] == 1 else info["H"] * info["V"]
        self.comp_of = [0 if c < hv else c - hv + 1 for c in range(self.bpm)]
        self.seg_start, self.seg_sub = [0], [0]
        for s in segs:
            self.seg_start.append(self.seg_start[-1] + 8 * len(s))
            self.seg_sub.append(self.seg_sub[-1] + max(1, -(-8 * len(s) // SUB_BITS)))
        self.nsub = self.seg_sub[-1]
        self.ngroups = -(-self.nsub // GROUP)
        self.sub_seg, self.sub_t, self.sub_start, self.sub_end = [], [], [], []
        for s in range(self.nseg):
            for t in range(self.seg_sub[s + 1] - self.seg_sub[s]):
                start = self.seg_start[s] + t * SUB_BITS
                self.sub_seg.append(s)
                self.sub_t.append(t)
                self.sub_start.append(start)
                self.sub_end.append(min(start + SUB_BITS, self.seg_start[s + 1]))
        # the 16 bits at every bit position (16 zero bytes follow the data, as in the workspace)
        bits = np.unpackbits(np.frombuffer(b"".join(segs) + bytes(16), np.uint8)).astype(np.int64)
        n = bits.size - 16
        w16 = sum(bits[i:i + n] << (15 - i) for i in range(16))
        done = {}
        self.dc_used, self.ac_used, self.ac_jump = [], [], []
        for c in range(info["nc"]):
            key = tuple(sorted(info["dc"][c].items()))
            if key not in done:
                length, sym = _lut(info["dc"][c])
                done[key] = (length[w16] + sym[w16]).tolist()
            self.dc_used.append(done[key])
            key = tuple(sorted(info["ac"][c].items())) + ("ac",)
            if key not in done:
                length, sym = _lut(info["ac"][c])
                r, sz = sym >> 4, sym & 15
                jump = np.where(sz > 0, r + 1, np.where(r == 15, 16, 64))      # min(k + jump, 64) is the next k
                done[key] = ((length[w16] + sz[w16]).tolist(), jump[w16].tolist())
            self.ac_used.append(done[key][0])
            self.ac_jump.append(done[key][1])
        self._memo = {}
        # the sequential decode: entry and exit state and completed blocks of every subsequence
        self.entry, self.exit, self.exact_cnt = [], [], []
        for s in range(self.nseg):
            st = (self.seg_start[s], 0, 0)
            for j in range(self.seg_sub[s], self.seg_sub[s + 1]):
                self.entry.append(st)
                p, c, k, cnt = self.run(j, st)
                st = (p, c, k)
                self.exit.append(st)
                self.exact_cnt.append(cnt)
        self.guess_cnt = [self.run(j, self.guess(j))[3] for j in range(self.nsub)]

    def guess(self, j):
        return (self.sub_start[j], 0, 0)

    def run(self, j, state, watch=-1):
        """decode_run<false> over subsequence j from `state`: (p, c, k, blocks completed).  watch: a bit position;
        the result is then whether a code word starts there"""
        key = (j,) + state
        if watch < 0 and key in self._memo:
            return self._memo[key]
        p, c, k = state
        end, bpm, comp_of = self.sub_end[j], self.bpm, self.comp_of
        done = 0
        while p < end:
            if p == watch:
                return True
            comp = comp_of[c]
            if k == 0:
                p += self.dc_used[comp][p]
                k = 1
                continue
            k += self.ac_jump[comp][p]
            p += self.ac_used[comp][p]
            if k >= 64:
                k = 0
                c = c + 1 if c + 1 < bpm else 0
                done += 1
        if watch >= 0:
            return False
        self._memo[key] = (p, c, k, done)
        return p, c, k, done

    def catch_up(self, j):
        """(n, met): a decode from the guess at subsequence j runs n subsequences before its state equals the
        sequential decode's at a subsequence end (met), or before its segment ends or n reaches CAP (not met)"""
        st = self.guess(j)
        if st == self.entry[j]:
            return 0, True
        last = self.seg_sub[self.sub_seg[j] + 1] - 1
        n = 0
        while True:
            st = self.run(j + n, st)[:3]
            n += 1
            if st == self.exit[j + n - 1]:
                return n, True
            if j + n - 1 == last or n == CAP:
                return n, False

    @functools.lru_cache(maxsize=None)
    def sync_group(self, w):
        """k_jd_sync's loop over workgroup w: (passes in which an entry changed, recorded entries, recorded counts)"""
        lo, hi = w * GROUP, min(w * GROUP + GROUP, self.nsub)
        ent = [self.guess(j) for j in range(lo, hi)]
        res = [self.run(j, e) for j, e in zip(range(lo, hi), ent)]
        passes = 0
        while True:
            new_ent, new_res = list(ent), list(res)
            for i in range(1, hi - lo):
                if self.sub_t[lo + i] > 0 and res[i - 1][:3] != ent[i]:
                    new_ent[i] = res[i - 1][:3]
                    new_res[i] = self.run(lo + i, new_ent[i])
            if new_ent == ent:
                return passes, ent, [r[3] for r in res]
            ent, res = new_ent, new_res
            passes += 1

    def seams(self):
        """what k_jd_seams does at every seam: the subsequences it walks, whether it reaches the end of its range,
        the subsequences among them whose recorded count is wrong, the correction of tail, the branch of tail_is_s
        and whether head chains over the tail of a workgroup that was itself corrected"""
        out = []
        for w in range(1, self.ngroups):
            jl = w * GROUP
            if self.sub_t[jl] == 0:
                continue
            s = self.sub_seg[jl]
            jend = min(self.seg_sub[s + 1], self.nsub, jl + GROUP) - 1
            _, ent, cnt = self.sync_group(w)
            j, delta, differs = jl, 0, 0
            while j <= jend and ent[j - jl] != self.entry[j]:
                delta += self.exact_cnt[j] - cnt[j - jl]
                differs += self.exact_cnt[j] != cnt[j - jl]
                j += 1
            out.append(dict(group=w, segment=s, walked=j - jl, to_end=j > jend, differs=differs, delta=delta,
                            tail_is_s=self.sub_seg[min(self.nsub, jl + GROUP) - 1] == s,
                            chained=self.sub_seg[jl - GROUP] == s and self.sub_t[jl - GROUP] > 0))
        return out

    def longest_gap(self):
        """the longest run of subsequences of one segment, its last left out, in which no block ends"""
        best = run = 0
        for j in range(self.nsub):
            if self.sub_t[j] == 0:
                run = 0
            if j + 1 == self.seg_sub[self.sub_seg[j] + 1]:
                continue
            run = run + 1 if self.exact_cnt[j] == 0 else 0
            best = max(best, run)
        return best

    def segment_bits(self):
        return [b - a for a, b in zip(self.seg_start, self.seg_start[1:])]

    def last_bit_alignments(self):
        """the byte offsets mod 4 of the segment starts whose segment has a full subsequence in which a code word of
        the sequential decode starts in the last bit: at offset 3 that code word reads the last word of the window"""
        got = set()
        for j in range(self.nsub):
            if self.sub_end[j] - self.sub_start[j] == SUB_BITS and self.run(j, self.entry[j], self.sub_end[j] - 1):
                got.add(self.seg_start[self.sub_seg[j]] // 8 % 4)
        return got


@functools.lru_cache(maxsize=None)
def sim(data):
    return Sim(data)


# ---- conditions on the inputs -----------------------------------------------------------------------------------------------
def model_blocks(data):
    """(blocks, 64) u8: every 8 x 8 block of the model's component planes, MCU padding included"""
    planes = dm._parsed_planes(bytes(data))[1]
    return np.concatenate([p.reshape(p.shape[0] // 8, 8, p.shape[1] // 8, 8).transpose(0, 2, 1, 3).reshape(-1, 64)
                           for p in planes])


def saturated_share(data):
    s = np.concatenate([p.reshape(-1) for p in dm.decode(data, "planes")])
    return float(np.mean((s == 0) | (s == 255)))


def figures(data):
    """the figures the host test prints for a file"""
    s = sim(data)
    inner = [j for j in range(s.nsub) if s.sub_t[j] > 0]
    never = sum(1 for j in inner if not s.catch_up(j)[1])
    return dict(subsequences=s.nsub, workgroups=s.ngroups, seams=len(s.seams()),
                never=never / len(inner) if inner else 0.0, gap=s.longest_gap(), segments=s.nseg,
                saturated=saturated_share(data))


# ---- A. never synchronising ---------------------------------------------------------------------------------------------------
Q2 = 2 * vf.ONES
# DC: the one symbol 4 on the 12-bit code 0; AC: run 0 size 4 on the same code, run 1 size 4 on the next
A_DC = sw.spec_from_lengths([4], [12])
A_AC = sw.spec_from_lengths([0x04, 0x14], [12, 12])


def dc_walk(rng, comp, lo, hi, seg_blocks=0):
    """DC values whose differences all have a magnitude in [lo, hi], each pulling the predictor towards 0; the
    predictor restarts every seg_blocks blocks"""
    pred, out = [0, 0, 0], []
    for b, c in enumerate(comp):
        if seg_blocks and b % seg_blocks == 0:
            pred = [0, 0, 0]
        d = int(rng.integers(lo, hi + 1))
        pred[c] += -d if pred[c] > 0 else d
        out.append(pred[c])
    return out


def a_blocks(n, comp, seed, seg_blocks=0):
    """n blocks of 61 symbols of 16 bits: DC, 57 coefficients at run 0 and three at run 1 (976 bits a block).  A
    guessed decode reads the same symbols in blocks of 61 from wherever it starts, so it keeps its distance; the 64
    symbols of a subsequence move the block ends by 3 symbols a subsequence and by 36 a workgroup, so the exact and
    the guessed decode complete different numbers of blocks in most workgroups (with one coefficient at run 1, 63
    symbols a block, a workgroup moves them by 4 and the two counts are equal 59 times in 63)"""
    rng = np.random.default_rng(seed)
    coefs = rng.integers(8, 16, (n, 64)) * rng.choice([-1, 1], (n, 64))
    coefs[:, [58, 60, 62]] = 0
    coefs[:, 0] = dc_walk(rng, comp, 8, 15, seg_blocks)
    return coefs


@functools.lru_cache(maxsize=None)
def a_file(sampling, w, h, seed, R=0):
    if sampling == "gray":
        n = -(-w // 8) * -(-h // 8)
        comp = np.zeros(n, np.int64)
        return sw.jpeg_file(w, h, a_blocks(n, comp, seed, R), comp, 1, qtabs={0: (0, Q2)}, dc={0: A_DC}, ac={0: A_AC}, R=R)
    assert sampling == "420"
    n = -(-w // 16) * -(-h // 16) * 6
    comp = np.tile([0, 0, 0, 0, 1, 2], n // 6)
    return sw.jpeg_file(w, h, a_blocks(n, comp, seed, 6 * R), comp, 6, H=2, V=2, qtabs=vf.q8(Q2, Q2), dc={0: A_DC, 1: A_DC},
                        ac={0: A_AC, 1: A_AC}, R=R)


A_GRAY = ("gray", 240, 240, 1)           # 900 blocks, 858 subsequences, 4 workgroups
A_420 = ("420", 160, 160, 2)             # 600 blocks, 572 subsequences, 3 workgroups


@functools.lru_cache(maxsize=None)
def group_a():
    return [Case("never gray 240x240", a_file(*A_GRAY), None, True),
            Case("never 420 160x160", a_file(*A_420), "NV12", True)]


def never_synchronises(data):
    """the properties of family A: (every seam is walked for 256 subsequences or to the end of its segment, some
    workgroup makes k_jd_sync loop its full 255 passes, every seam walks over a wrong recorded count)"""
    s = sim(data)
    seams = s.seams()
    return (bool(seams) and all(x["walked"] >= GROUP or x["to_end"] for x in seams)
            and all(not s.catch_up(x["group"] * GROUP)[1] for x in seams),
            any(s.sync_group(w)[0] == GROUP - 1 for w in range(s.ngroups)),
            bool(seams) and all(x["differs"] > 0 for x in seams))


@functools.lru_cache(maxsize=None)
def noise_twin():
    """the Annex K q100 noise file of A's gray size: the same kernels, and it synchronises at once"""
    return vf.writer_file(A_GRAY[1], A_GRAY[2], "gray", 7)


# ---- B. blocks longer than a subsequence ------------------------------------------------------------------------------------
B_DC = sw.table_spec(list(range(12)), "deep_dc")                                # size 11 on a 16-bit code
B_AC = sw.table_spec([s for s in vf.AC_SYMBOLS if s != 0x0A][:14] + [0x0A]
                     + [s for s in vf.AC_SYMBOLS if s != 0x0A][14:], "deep_ac")    # run 0 size 10 on a 16-bit code
B_SIZE = (136, 136)
B_FIRST = 4              # found by search_b_first()


@functools.lru_cache(maxsize=None)
def b_file(first, seed=3):
    """gray, 289 blocks of 1665 bits: a DC difference of size 11 and 63 coefficients of size 10, all on 16-bit codes.
    Block 0 has only `first` coefficients and an EOB, which sets where the block ends fall among the subsequences"""
    w, h = B_SIZE
    n = -(-w // 8) * -(-h // 8)
    rng = np.random.default_rng(seed)
    comp = np.zeros(n, np.int64)
    coefs = rng.integers(512, 1024, (n, 64)) * rng.choice([-1, 1], (n, 64))
    coefs[:, 0] = dc_walk(rng, comp, 1024, 2047)
    coefs[0, 1 + first:] = 0
    return sw.jpeg_file(w, h, coefs, comp, 1, qtabs={0: (0, vf.ONES)}, dc={0: B_DC}, ac={0: B_AC})


def long_block_props(data):
    """(subsequences of the sequential decode in which no block ends, those among them that are the first of a
    workgroup and no segment start)"""
    s = sim(data)
    empty = [j for j in range(s.nsub) if s.exact_cnt[j] == 0 and j + 1 != s.seg_sub[s.sub_seg[j] + 1]]
    return empty, [j for j in empty if j % GROUP == 0 and s.sub_t[j] > 0]


def search_b_first():
    """the search that gave B_FIRST: the first length of block 0 with which the first subsequence of workgroup 1
    holds no block end"""
    for first in range(63):
        if long_block_props(b_file(first))[1]:
            return first
    return None


@functools.lru_cache(maxsize=None)
def group_b():
    return [Case("long blocks gray 136x136", b_file(B_FIRST), None, False)]


# ---- C. restart structure -----------------------------------------------------------------------------------------------------
Q3 = 3 * vf.ONES


def sparse_blocks(n, comp, seed):
    """n small blocks for the Annex K tables: a DC value and three coefficients among the first twenty"""
    rng = np.random.default_rng(seed)
    coefs = np.zeros((n, 64), np.int64)
    coefs[:, 0] = rng.integers(-96, 97, n)
    for b in range(n):
        coefs[b, rng.choice(np.arange(1, 21), 3, replace=False)] = rng.integers(1, 32, 3) * rng.choice([-1, 1], 3)
    return coefs


@functools.lru_cache(maxsize=None)
def many_segments(sampling, w, h, seed):
    """R = 1: one segment and one subsequence per MCU"""
    if sampling == "gray":
        n = -(-w // 8) * -(-h // 8)
        comp = np.zeros(n, np.int64)
        return sw.jpeg_file(w, h, sparse_blocks(n, comp, seed), comp, 1, qtabs={0: (0, Q3)}, R=1)
    n = -(-w // 16) * -(-h // 16) * 6
    comp = np.tile([0, 0, 0, 0, 1, 2], n // 6)
    return sw.jpeg_file(w, h, sparse_blocks(n, comp, seed), comp, 6, H=2, V=2, qtabs=vf.q8(Q3, Q3), R=1)


# segments of an exact length: DC 16 bits, run 0 size 4 16 bits, run 0 size 3 15 bits, EOB 8 bits
L_DC = A_DC
L_AC = sw.spec_from_lengths([0x00, 0x04, 0x03], [8, 12, 12])
LENGTHS_SMALL = (48, 24, 3, (1024, 1016, 1032, 2048, 2040, 2056))                  # w, h, R, bits of every segment
LENGTHS_LARGE = (208, 240, 260, (1024 * 256, 1024 * 256 + 8, 1024 * 256 - 8))


@functools.lru_cache(maxsize=None)
def lengths_file(w, h, R, targets, seed=5):
    """gray, every segment R blocks that end in an EOB, their coefficients counted out so that segment i has exactly
    targets[i] bits (a multiple of 8: no padding bits)"""
    rng = np.random.default_rng(seed)
    assert -(-w // 8) * -(-h // 8) == R * len(targets)
    rows = []
    for bits in targets:
        body = bits - 24 * R                                   # beyond a DC symbol and an EOB per block
        total = -(-body // 16)
        short = 16 * total - body                              # coefficients of size 3: one bit less each
        for i in range(R):
            n = total // R + (i < total % R)
            assert short <= n <= 62
            z = np.zeros(64, np.int64)
            z[1:1 + n] = rng.integers(8, 16, n) * rng.choice([-1, 1], n)
            if i == 0:
                z[1:1 + short] = rng.integers(4, 8, short) * rng.choice([-1, 1], short)
            rows.append(z)
    coefs = np.array(rows)
    comp = np.zeros(len(rows), np.int64)
    coefs[:, 0] = dc_walk(rng, comp, 8, 15, R)
    return sw.jpeg_file(w, h, coefs, comp, 1, qtabs={0: (0, Q2)}, dc={0: L_DC}, ac={0: L_AC}, R=R)


# A's stream in segments of 420 blocks: 414 subsequences, 1.6 workgroups; two segments
A_SEGMENTED = ("gray", 224, 240, 4, 420)

# (seed) of 64 x 64 gray q100 noise files with R = 4, found by search_last_bit_seeds(): between them a code word starts
# in the last bit of a full subsequence for segment starts at byte 0, 1, 2 and 3 mod 4
LAST_BIT_SEEDS = (0, 1, 2)


def last_bit_file(seed):
    return vf.writer_file(64, 64, "gray", seed, R=4)


def search_last_bit_seeds(limit=200):
    """the search that gave LAST_BIT_SEEDS: the first seeds that add an alignment not yet covered"""
    found, missing = [], {0, 1, 2, 3}
    for seed in range(limit):
        new = Sim(last_bit_file(seed)).last_bit_alignments() & missing
        if new:
            found.append(seed)
            missing -= new
        if not missing:
            break
    return found, missing


@functools.lru_cache(maxsize=None)
def group_c():
    cases = [Case("1089 segments gray 264x264", many_segments("gray", 264, 264, 11), None, True),
             Case("2116 segments gray 368x368", many_segments("gray", 368, 368, 12), None, True),
             Case("1056 segments 420 528x512", many_segments("420", 528, 512, 13), "NV12", True),
             Case("segment lengths m 1 2", lengths_file(*LENGTHS_SMALL), None, True),
             Case("segment lengths m 256", lengths_file(*LENGTHS_LARGE), None, True),
             Case("never gray, 1.6 workgroups a segment", a_file(*A_SEGMENTED), None, True)]
    return cases + [Case(f"last bit seed {s}", last_bit_file(s), None, True) for s in LAST_BIT_SEEDS]


# ---- D. a batch ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def group_d():
    """multi-workgroup files next to files of one subsequence; the test also runs it reversed"""
    big = group_a() + group_b() + [c for c in group_c() if "lengths m 256" in c.name or "1.6" in c.name
                                  or "1089" in c.name]
    cases = []
    for i, c in enumerate(big):
        w, h = ((1, 1), (7, 9), (17, 33))[i % 3]
        sampling = ("420", "gray", "444")[i % 3]
        small = jf.pillow_file(jf.picture(w, h, "noise", 20 + i), sampling, 90)
        cases += [Case(f"small {sampling} {w}x{h}", small, None, True), c._replace(raw=None)]
    return cases + [cases[0]]


# ---- E. one corrupt file --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def corrupt_pair():
    """(good, bad): A's gray file, and the same with one bit flipped in its last workgroup: coefficient 30 of the
    fifth-last block gets the code of run 1, so the block's last symbol, a run of 1 from 63, runs past 63.  The A
    stream has no FF byte, so its bytes are the unstuffed ones"""
    good = a_file(*A_GRAY)
    a, b = sw.entropy_bounds(good)
    assert b"\xff" not in good[a:b] and (b - a) % 122 == 0
    at = a + (b - a) - 5 * 122 + 2 * 30 + 1                      # low byte of that symbol: 4 code bits, 4 value bits
    assert good[at] >> 4 == 0
    bad = good[:at] + bytes([good[at] | 0x10]) + good[at + 1:]
    return good, bad
