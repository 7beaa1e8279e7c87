"""CPU model of the self-synchronising entropy decode of k_jpeg.hip: how many passes a stream needs at a given chunk size.

TEST INFRASTRUCTURE ONLY.  A plain Python restatement of what k_jpeg.hip's header comment and jrun specify, nothing of the device
code is called:
  - marker parse, byte destuffing (FF00 -> FF, the data ends at the first other marker) and the canonical Huffman tables of T.81
    Annex C;
  - the decoder state at a symbol boundary: (bit position in the destuffed segment, zigzag index k, block in the MCU);
  - a symbol belongs to the chunk its first bit lies in: a chunk's decoder goes on while its position is in front of the chunk's end
    and publishes the state in which it left;
  - a prefix that is no code reads as a 16-bit EOB (in DC position: a 16-bit zero difference), bits behind the segment read as zeros;
  - the Jacobi iteration: pass 0 decodes every chunk from the guess (chunk start, k = 0, block 0) - chunk 0 from the truth; in pass
    n > 0 every chunk whose predecessor published, up to pass n - 1, another state than the one the chunk last started from decodes
    again from it.  The first pass that changes no published state is the fixed point.

Its only job is to choose and to justify test inputs (tests/golden/make_golden_jpeg_edges.py, tests/test_gpu_jpeg_edges.py): which
streams keep the host loop of jdecode_staged busy for how long.  Pass counts of the device are NOT compared with it exactly: a
device pass may read a predecessor state written in the same launch and so be ahead of the Jacobi schedule, never behind it.

Streams without restart intervals are enough for that and all this model reads: a stream with a DRI segment is refused.
"""
import numpy as np

class Scan:
    """What the decoders of one stream share: the destuffed entropy segment, per block of an MCU the (DC, AC) look-up tables, and
    the geometry.  A table maps the next 16 bits to (code length << 8) | symbol; no code under the prefix: (16 << 8) | 0."""

    def __init__(self, h, w, ncomp, hs, vs, tables, ent):
        self.h, self.w, self.ncomp, self.hmax, self.vmax = h, w, ncomp, hs, vs
        self.mcux, self.mcuy = -(-w // (8 * hs)), -(-h // (8 * vs))
        comp = [0] * (hs * vs) + ([1, 2] if ncomp == 3 else [])
        self.bpm = len(comp)
        self.nblk = self.mcux * self.mcuy * self.bpm
        self.tab = [tables[c] for c in comp]                     # [block in MCU] -> (dc lut, ac lut)
        self.ent = ent
        self._pad = ent + bytes(8)


def _lut(bits, vals):
    """T.81 Annex C code assignment, as a 65536-entry table over the next 16 bits."""
    lut = np.full(65536, 16 << 8, np.int32)
    code, p = 0, 0
    for l in range(1, 17):
        for _ in range(bits[l - 1]):
            lo = code << (16 - l)
            if lo < 65536:                                       # (an over-subscribed table: no bit pattern reaches the code)
                lut[lo:lo + (1 << (16 - l))] = (l << 8) | vals[p]
            code += 1; p += 1
        code <<= 1
    return lut.tolist()


def parse(data):
    """Scan of a baseline stream with one interleaved scan, gray or YCbCr with 1x1 chroma; ValueError otherwise."""
    data = bytes(data)
    if data[:2] != b"\xff\xd8":
        raise ValueError("no SOI")
    i, huff, frame, sel = 2, {}, None, None
    while True:
        if data[i] != 0xFF:
            raise ValueError("marker expected")
        m, L = data[i + 1], (data[i + 2] << 8) | data[i + 3]
        s = data[i + 4:i + 2 + L]
        if m == 0xC4:
            k = 0
            while k < len(s):
                tc_th, bits = s[k], list(s[k + 1:k + 17])
                n = sum(bits)
                huff[tc_th] = _lut(bits, list(s[k + 17:k + 17 + n]))
                k += 17 + n
        elif m in (0xC0, 0xC1):
            h, w, nc = (s[1] << 8) | s[2], (s[3] << 8) | s[4], s[5]
            samp = [(s[7 + 3 * c] >> 4, s[7 + 3 * c] & 15) for c in range(nc)]
            if nc not in (1, 3) or any(x != (1, 1) for x in samp[1:]):
                raise ValueError("unsupported frame")
            frame = (h, w, nc) + (samp[0] if nc == 3 else (1, 1))
        elif 0xC2 <= m <= 0xCF and m not in (0xC8, 0xCC):
            raise ValueError("not baseline Huffman")
        elif m == 0xDD:
            if (s[0] << 8) | s[1]:
                raise ValueError("restart intervals are outside this model")
        elif m == 0xDA:
            if frame is None or s[0] != frame[2]:
                raise ValueError("one interleaved scan expected")
            sel = [(s[2 + 2 * c] >> 4, s[2 + 2 * c] & 15) for c in range(frame[2])]
            i += 2 + L
            break
        i += 2 + L
    out = bytearray()
    while i < len(data):                                         # destuffing; any marker ends the data
        j = data.find(b"\xff", i)
        if j < 0:
            out += data[i:]; break
        out += data[i:j]
        if j + 1 >= len(data) or data[j + 1] == 0:
            out.append(0xFF); i = j + 2
        else:
            break
    tables = [(huff[td], huff[0x10 | ta]) for td, ta in sel]
    return Scan(*frame, tables, bytes(out))


def run(scan, state, bend):
    """Decodes symbols from `state` = (bit, k, blk) while they start in front of bit `bend`: (state left in, blocks completed)."""
    bp, k, blk = state
    d, tab, bpm, done = scan._pad, scan.tab, scan.bpm, 0
    nbits = len(scan.ent) * 8
    while bp < bend:
        if bp < nbits:
            p = bp >> 3
            top = (((d[p] << 16) | (d[p + 1] << 8) | d[p + 2]) >> (8 - (bp & 7))) & 0xFFFF
        else:
            top = 0
        e = tab[blk][1 if k else 0][top]
        ln, sym = e >> 8, e & 255
        s, r = sym & 15, sym >> 4
        bp += ln + s
        k += 1 if not k else r + 1 if s else 16 if r == 15 else 64
        if k >= 64:
            k = 0
            blk = blk + 1 if blk + 1 < bpm else 0
            done += 1
    return (bp, k, blk), done


def chunk_count(scan, jch):
    return len(scan.ent) // jch + 1


def serial(scan, jch):
    """One decoder from the true start through every chunk: (entry state per chunk, blocks completed per chunk, bit position at
    which block scan.nblk was complete or None)."""
    nch, cbits = chunk_count(scan, jch), jch * 8
    entry, counts, st = [], [], (0, 0, 0)
    for i in range(nch):
        entry.append(st)
        st, n = run(scan, st, (i + 1) * cbits)
        counts.append(n)
    # where the last block of the frame ends: one more walk, symbol by symbol (cheap: only used by the tests of the model)
    st, done, end = (0, 0, 0), 0, None
    while done < scan.nblk and st[0] < nch * cbits:
        st2, n = run(scan, st, st[0] + 1)                        # one symbol
        done += n
        st = st2
        if done == scan.nblk:
            end = st[0]
    return entry, counts, end


def iterate(scan, jch, max_passes=None):
    """The Jacobi iteration.  Returns dict(chunks, passes, entry, counts): passes = the number of the first pass (pass 0 = the
    guesses) that changed no published state - the pass whose flag the host loop finds clear; entry / counts = the state every chunk
    last started from and the blocks it completed then."""
    nch, cbits = chunk_count(scan, jch), jch * 8
    used = [(i * cbits, 0, 0) for i in range(nch)]
    res = [run(scan, used[i], (i + 1) * cbits) for i in range(nch)]
    state, counts = [r[0] for r in res], [r[1] for r in res]
    n = 0
    while True:
        n += 1
        if max_passes is not None and n > max_passes:
            raise RuntimeError("no fixed point")
        prev, changed = list(state), False
        for i in range(1, nch):
            if prev[i - 1] != used[i]:
                used[i] = prev[i - 1]
                x, counts[i] = run(scan, used[i], (i + 1) * cbits)
                if x != state[i]:
                    state[i], changed = x, True
        if not changed:
            return dict(chunks=nch, passes=n, entry=used, counts=counts)


def passes(stream, jch=64):
    """(chunks, passes) of a JPEG stream at `jch` entropy bytes per decoder: see iterate."""
    r = iterate(parse(stream), jch)
    return r["chunks"], r["passes"]


def host_loop(quiet_pass, nch_max, slots=64, clear_reused_slot=True):
    """The host loop of jdecode_staged over a batch whose passes 1 .. quiet_pass - 1 each change some published state and whose
    later passes change none (what iterate reports for the batch's slowest stream): seven passes before the first look at the
    flags, then four at a time; one flag slot per pass up to slots - 1, the last slot cleared in front of and reused by every pass
    from `slots` on; gives up behind pass nch_max + 2.  Returns (passes queued, "converged" | "guard").
    clear_reused_slot=False is the loop WITHOUT the memset between the tail passes: what the slow-stream tests would meet then."""
    if nch_max == 1:
        return 0, "converged"
    flags, it = [0] * slots, 0
    while True:
        first = it + 1
        for _ in range(7 if it == 0 else 4):
            it += 1
            if it >= slots and clear_reused_slot:
                flags[slots - 1] = 0
            if it < quiet_pass:
                flags[min(it, slots - 1)] = 1
        if any(not flags[min(k, slots - 1)] for k in range(first, it + 1)):
            return it, "converged"
        if it > nch_max + 2:
            return it, "guard"
