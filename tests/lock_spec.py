"""The frame lock's contract, in plain NumPy and a serial loop: the reference decoder's loop with its flywheel
(decoder/src/newdecoder.cpp:212-270 with :218-237 and :321-338, flywheelRecheck = R, parameters.h:41: 4), where the range
a chunk is correlated over depends on the Reed-Solomon outcome of the frame before it.  It stands on framer_spec (the
rows, the oracle's correlator) and on ccsds (the decoder's stages).

State: the cursor c and the symbols from c on; ok = False (lastFrameOK), fc = 0 (flywheelCount); the decoder's carry of
64 symbols.  While c + F <= end, with the state as it was at the chunk's entry:

 1. fc == R: ok = False, fc = 0                                                                      (:218-221)
 2. not ok: hit = correlate(stream[c : c + F]), positions 0 .. F - 65 (mode FULL).  Otherwise
    hit = correlate(stream[c : c + F // 16]), positions 0 .. F // 16 - 65: position 0 keeps it (mode SHORT), any other
    position takes the full-range hit instead, ok = False, fc = 0 (mode MISS)                       (:224-236)
 3. fc += 1
 4. hit.correlation < 46: a row (hit, valid = 0, zero frame, start = c); c += F; ok is NOT touched   (:244-247)
 5. else if c + hit.position + F > end: stop; nothing is emitted or consumed and ok, fc go back to their values at the
    chunk's entry (the chunk is walked again in the next call)
 6. else a row (hit, valid = 1, start = c + hit.position, the frame inverted when hit.word != 0 on LRIT), decoded behind
    the carry as the frame decoder does; ok = info.ok (:321-338); c = start + F

Per row: the framer's four outputs, the decoder's three, and a mode byte FULL / SHORT / MISS, plus RECHECK when step 1
fired on the chunk.  `hits` holds the hit that was used (the short one under SHORT).

decode(frame, carry) -> (cadu, block, info record) is the decoder on one valid frame; the default is ccsds's stages, a
test of the state machine alone may pass a cheap one with small frames (frame >= 1040, so that frame // 16 >= 65)."""
import numpy as np

import ccsds
import framer_spec as fs

FULL, SHORT, MISS, RECHECK = 0, 1, 2, 4
RECHECK_DEFAULT = 4                                         # decoder/src/parameters.h:41
INFO_DTYPE = np.dtype([("valid", np.uint32), ("ok", np.uint32), ("viterbi_errors", np.uint32),
                       ("rs_errors", np.int32, (4,)), ("scid", np.uint32), ("vcid", np.uint32), ("counter", np.uint32)])
STATS = fs.STATS + ("short_kept", "short_missed", "rechecks", "sensitive_chunks", "frames_ok", "frames_bad")
FIELDS = ("frames", "valid", "hits", "start", "mode", "cadu", "block", "info")


def absent_info():
    z = np.zeros((), INFO_DTYPE)
    z["rs_errors"] = -1
    return z


def make_ccsds_decode(hrit):
    """The frame decoder's stages on one valid frame behind `carry` ("Frame decoder")."""
    def decode(frame, carry):
        w, _, _ = ccsds.windows(frame[None, :], [1], carry)
        bits, err = ccsds.viterbi_batch(w)
        cadu = ccsds.cadu_from_bits(bits, hrit)[0]
        block, n, ok = ccsds.rs_decode_blocks(ccsds.derandomize(cadu[4:])[None, :])
        scid, vcid, counter = ccsds.header_fields(block)
        info = np.zeros((), INFO_DTYPE)
        info["valid"], info["ok"], info["viterbi_errors"] = 1, int(ok[0]), int(err[0])
        info["rs_errors"] = n[0]
        info["scid"], info["vcid"], info["counter"] = int(scid[0]), int(vcid[0]), int(counter[0])
        return cadu, block[0], info
    return decode


class Rows:
    def __init__(self, frame, **kw):
        zero = dict(frames=np.zeros((0, frame), np.int8), valid=np.zeros(0, np.uint8), hits=np.zeros((0, 4), np.uint32),
                    start=np.zeros(0, np.uint64), mode=np.zeros(0, np.uint8), cadu=np.zeros((0, ccsds.CADU_BYTES), np.uint8),
                    block=np.zeros((0, ccsds.BLOCK_BYTES), np.uint8), info=np.zeros(0, INFO_DTYPE))
        for f in FIELDS:
            setattr(self, f, kw.get(f, zero[f]))

    def __len__(self):
        return len(self.valid)

    @staticmethod
    def concat(parts, frame):
        parts = [p for p in parts if len(p)]
        if not parts:
            return Rows(frame)
        return Rows(frame, **{f: np.concatenate([getattr(p, f) for p in parts]) for f in FIELDS})

    def same_as(self, other):
        return all(np.array_equal(getattr(self, f), getattr(other, f)) for f in FIELDS)


class Lock:
    """cache: a dict shared by locks that are fed the SAME stream with the same decode; it holds the correlations
    (cursor, range) -> hit and the decoded frames (start, inverted, carry) -> outputs."""

    def __init__(self, hrit=False, recheck=RECHECK_DEFAULT, frame=fs.FRAME, decode=None, cache=None):
        import oracle
        if not 1 <= int(recheck) <= 255:
            raise ValueError("recheck: 1 .. 255")
        if frame // 16 < 65:
            raise ValueError("frame >= 1040")
        self._correlate = oracle.sync_correlate
        self.hrit = bool(hrit)
        self.words = fs.HRIT_WORDS if hrit else fs.LRIT_WORDS
        self.frame = int(frame)
        self.recheck = int(recheck)
        self.decode = decode or make_ccsds_decode(self.hrit)
        self.cache = cache
        self.reset()

    def reset(self):
        self.cursor = self.end = 0
        self.buf = np.zeros(0, np.int8)
        self.ok, self.fc = False, 0
        self.dcarry = np.zeros(ccsds.CARRY, np.int8)
        self.counts = dict.fromkeys(STATS, 0)

    def _hit(self, c, base, span):
        key = (c, span)
        if self.cache is not None and key in self.cache:
            return self.cache[key]
        chunk = self.buf[c - base:c - base + span]
        hit = tuple(int(v) for v in self._correlate(chunk, self.words, span)[0])
        if self.cache is not None:
            self.cache[key] = hit
        return hit

    def _decode(self, start, inverted, frame):
        key = ("d", start, inverted, self.dcarry.tobytes())
        if self.cache is not None and key in self.cache:
            return self.cache[key]
        out = self.decode(frame, self.dcarry)
        if self.cache is not None:
            self.cache[key] = out
        return out

    def push(self, symbols):
        F, R, n = self.frame, self.recheck, self.counts
        new = np.ascontiguousarray(symbols, np.int8).reshape(-1)
        self.buf = np.concatenate([self.buf, new])
        self.end += len(new)
        base = c = self.cursor
        out = {f: [] for f in FIELDS}
        while c + F <= self.end:
            ok0, fc0 = self.ok, self.fc
            seen = dict(n)
            recheck = self.fc == R
            if recheck:
                self.ok, self.fc = False, 0
                n["rechecks"] += 1
            if not self.ok:
                hit, mode = self._hit(c, base, F), FULL
            else:
                hit, mode = self._hit(c, base, F // 16), SHORT
                if hit[1] != 0:
                    hit, mode = self._hit(c, base, F), MISS
                    self.ok, self.fc = False, 0
                    n["short_missed"] += 1
                else:
                    n["short_kept"] += 1
            # sensitive: full position not 0, short position 0, fc != R at entry -- whatever ok is (a counter only)
            if not recheck and self._hit(c, base, F)[1] != 0 and self._hit(c, base, F // 16)[1] == 0:
                n["sensitive_chunks"] += 1
            self.fc += 1
            word, pos, corr = hit
            if corr < fs.MIN_CORRELATION:
                out["frames"].append(np.zeros(F, np.int8))
                out["valid"].append(0)
                out["hits"].append((word, pos, corr, 0))
                out["start"].append(c)
                out["mode"].append(mode | (RECHECK if recheck else 0))
                out["cadu"].append(np.zeros(ccsds.CADU_BYTES, np.uint8))
                out["block"].append(np.zeros(ccsds.BLOCK_BYTES, np.uint8))
                out["info"].append(absent_info())
                n["dropped_chunks"] += 1
                c += F
                continue
            if c + pos + F > self.end:
                self.ok, self.fc = ok0, fc0
                self.counts = n = seen
                break
            s = c + pos
            fr = self.buf[s - base:s - base + F].copy()
            inverted = word != 0 and not self.hrit
            if inverted:
                fr = (fr.view(np.uint8) ^ 0xFF).view(np.int8)
            cadu, block, info = self._decode(s, inverted, fr)
            self.dcarry = fr[-ccsds.CARRY:].copy()
            out["frames"].append(fr)
            out["valid"].append(1)
            out["hits"].append((word, pos, corr, 0))
            out["start"].append(s)
            out["mode"].append(mode | (RECHECK if recheck else 0))
            out["cadu"].append(cadu)
            out["block"].append(block)
            out["info"].append(info)
            n["frames"] += 1
            n["resyncs"] += 1 if pos != 0 else 0
            n["frames_ok" if info["ok"] else "frames_bad"] += 1
            self.ok = bool(info["ok"])
            c = s + F
        self.buf = self.buf[c - base:].copy()
        self.cursor = c
        n["rows"] += len(out["valid"])
        assert len(self.buf) <= 2 * F - 66 and len(out["valid"]) <= fs.rows_cap(len(new), F)
        if not out["valid"]:
            return Rows(F)
        return Rows(F, frames=np.stack(out["frames"]), valid=np.array(out["valid"], np.uint8),
                    hits=np.array(out["hits"], np.uint32).reshape(-1, 4), start=np.array(out["start"], np.uint64),
                    mode=np.array(out["mode"], np.uint8), cadu=np.stack(out["cadu"]), block=np.stack(out["block"]),
                    info=np.array(out["info"], INFO_DTYPE))

    @property
    def carry(self):
        return len(self.buf)

    def stats(self):
        return dict(self.counts, symbols=self.end, cursor=self.cursor, carry=self.carry)


def walk(stream, cuts=(), **kw):
    """The stream pushed in the pieces the cuts make: (all rows, the rows of each call, the lock)."""
    lk = Lock(**kw)
    stream = np.ascontiguousarray(stream, np.int8)
    edges = [0] + [int(c) for c in cuts] + [len(stream)]
    per_call = [lk.push(stream[a:b]) for a, b in zip(edges[:-1], edges[1:])]
    return Rows.concat(per_call, lk.frame), per_call, lk
