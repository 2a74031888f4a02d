"""The stream frame synchroniser's contract, in plain NumPy and a serial loop: the reference decoder's walk over a stream
of int8 soft symbols, chunk by chunk (decoder/src/newdecoder.cpp:212-270 with flywheelRecheck = 1).  The per-chunk
primitive is the oracle's correlator on stream[c : c + F], so this specification stands on the oracle the fixed-window
correlator is already held to.

State: the cursor c (absolute offset, 0 at start) and the symbols from c on that are not consumed yet.  While
c + F <= end (the symbols received so far):

 1. hit = oracle.sync_correlate(stream[c : c + F]): positions 0 .. F - 65; per word the greatest agreement and the FIRST
    position that reaches it; across words the FIRST word with the strictly greatest count; no agreeing bit at all
    reports position 0, word 0.
 2. hit.correlation < min_correlation: a row (hit, valid = 0, zero frame, start = c); c += F           (:244-247)
 3. else if c + hit.position + F > end: stop -- the chunk is walked again when more symbols have arrived, nothing is
    emitted or consumed for it (the reference blocks in Receive)
 4. else: a row (hit, valid = 1, start = c + hit.position, frame = stream[start : start + F], every byte XOR 0xFF
    when hit.word != 0 on a LRIT framer -- HRIT never inverts, :266-270); c = start + F

Consequences (tests/test_framer_spec.py): the rows do not depend on where the stream is cut into calls; the carry after a
call is at most 2 F - 66 bytes; a call of n symbols emits at most rows_cap(n) = (n + 2 F - 66) // F rows."""
import numpy as np

LRIT_WORDS = (0xfca2b63db00d9794, 0x035d49c24ff2686b)       # decoder/src/newdecoder.cpp:21-24
HRIT_WORDS = (0xfc4ef4fd0cc2df89, 0x25010b02f33d2076)
FRAME = 16384
MIN_CORRELATION = 46

STATS = ("symbols", "cursor", "rows", "frames", "dropped_chunks", "resyncs", "carry")


def rows_cap(n, frame=FRAME):
    return (n + 2 * frame - 66) // frame


class Rows:
    """The rows of one call (or of several, concatenated)."""

    def __init__(self, frame, frames=None, valid=None, hits=None, start=None):
        self.frames = np.zeros((0, frame), np.int8) if frames is None else frames
        self.valid = np.zeros(0, np.uint8) if valid is None else valid
        self.hits = np.zeros((0, 4), np.uint32) if hits is None else hits      # word, position, correlation, 0
        self.start = np.zeros(0, np.uint64) if start is None else start

    def __len__(self):
        return len(self.valid)

    @staticmethod
    def concat(parts, frame):
        parts = [p for p in parts if len(p)]
        if not parts:
            return Rows(frame)
        return Rows(frame, *(np.concatenate([getattr(p, f) for p in parts]) for f in ("frames", "valid", "hits", "start")))


class Framer:
    """cache: a dict shared by framers that are fed the SAME stream (cursor -> hit); the correlation of a chunk depends
    on its bytes alone, so a second cutting of one stream need not ask the oracle again."""

    def __init__(self, hrit=False, frame=FRAME, min_correlation=MIN_CORRELATION, cache=None):
        import oracle
        self._correlate = oracle.sync_correlate
        self.hrit = bool(hrit)
        self.words = HRIT_WORDS if hrit else LRIT_WORDS
        self.frame = int(frame)
        self.min_correlation = int(min_correlation)
        self.cache = cache
        self.reset()

    def reset(self):
        self.cursor = 0                         # absolute
        self.end = 0                            # symbols received
        self.buf = np.zeros(0, np.int8)         # stream[cursor : end]
        self.rows = self.frames = self.dropped = self.resyncs = 0

    def push(self, symbols):
        F = self.frame
        new = np.ascontiguousarray(symbols, np.int8).reshape(-1)
        self.buf = np.concatenate([self.buf, new])
        self.end += len(new)
        base = self.cursor                      # absolute offset of buf[0] during this call
        c = self.cursor
        frames, valid, hits, start = [], [], [], []
        while c + F <= self.end:
            word, pos, corr = self._hit_at(c, base)
            if corr < self.min_correlation:
                frames.append(np.zeros(F, np.int8))
                valid.append(0)
                hits.append((word, pos, corr, 0))
                start.append(c)
                self.dropped += 1
                c += F
                continue
            if c + pos + F > self.end:
                break
            s = c + pos
            fr = self.buf[s - base:s - base + F].copy()
            if word != 0 and not self.hrit:
                fr = (fr.view(np.uint8) ^ 0xFF).view(np.int8)
            frames.append(fr)
            valid.append(1)
            hits.append((word, pos, corr, 0))
            start.append(s)
            self.frames += 1
            self.resyncs += 1 if pos != 0 else 0
            c = s + F
        self.buf = self.buf[c - base:].copy()
        self.cursor = c
        self.rows += len(valid)
        assert len(self.buf) <= 2 * F - 66 and len(valid) <= rows_cap(len(new), F)
        if not valid:
            return Rows(F)
        return Rows(F, np.stack(frames), np.array(valid, np.uint8), np.array(hits, np.uint32).reshape(-1, 4),
                    np.array(start, np.uint64))

    def _hit_at(self, c, base):
        if self.cache is not None and c in self.cache:
            return self.cache[c]
        chunk = self.buf[c - base:c - base + self.frame]
        word, pos, corr = (int(v) for v in self._correlate(chunk, self.words, self.frame)[0])
        if self.cache is not None:
            self.cache[c] = (word, pos, corr)
        return word, pos, corr

    @property
    def carry(self):
        return len(self.buf)

    def stats(self):
        return dict(symbols=self.end, cursor=self.cursor, rows=self.rows, frames=self.frames, dropped_chunks=self.dropped,
                    resyncs=self.resyncs, carry=self.carry)


def walk(stream, cuts=(), **kw):
    """The stream pushed in the pieces the cuts make: (all rows, the rows of each call, the framer)."""
    fr = Framer(**kw)
    stream = np.ascontiguousarray(stream, np.int8)
    edges = [0] + [int(c) for c in cuts] + [len(stream)]
    per_call = [fr.push(stream[a:b]) for a, b in zip(edges[:-1], edges[1:])]
    return Rows.concat(per_call, fr.frame), per_call, fr
