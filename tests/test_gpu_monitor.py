"""GPU tier: the link monitor (xrit_monitor_*, LinkMonitor) against the specification of tests/monitor_spec.py.  Everything
the stage sums is an integer, so every comparison here is np.array_equal on the rows, the summary and the state, the
histogram included: both symbol types, blocks of 64, 192 and 1984 (a wave per piece), 2048, 16384, 32704 and 32768 (a
workgroup per piece), the sizes around a block, source offsets that move the 16-byte core against the block boundaries, a
push of 4100 pieces on the workgroup path's grid of 2048, constructed values (NaN, infinities, signed zeros, the clamp's
edges, ties, a denormal, s4 next to 2^63), each of them in front of a 16-byte group's first symbol, of a block's first and
of a call's first, a stream cut into calls, reset, two handles, a refused
call, the stage behind the chain and behind the quantiser on one stream, the host forms and xrit_demod_host --monitor."""
import os
import subprocess

import numpy as np
import pytest

import monitor_spec as sp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# 192: 12 int8 groups for a wave's 64 lanes; 1984 and 2048: either side of the switch from a wave to a workgroup per piece (1984:
# 7.75 trips of the wave's 16-byte loop); 32704: the largest block that is no power of two
BLOCKS = (64, 192, 1984, 2048, 16384, 32704, 32768)
LEADS = {sp.F32: (0, 4, 12), sp.I8: (0, 1, 3, 15)}
N_STREAM = 100003
_STREAMS = {}


@pytest.fixture(scope="module")
def xa():
    import xritdemod_amd
    xritdemod_amd.lib()
    if xritdemod_amd.device_count() < 1:
        pytest.fail("the -m gpu tier needs a HIP device; the library has no CPU path")
    return xritdemod_amd


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.fixture(autouse=True)
def hand_memory_back(torch):
    """The tests after these run on the same device: every test here returns what it cached."""
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def stream(symbol_type, n=N_STREAM):
    """BPSK at 0.4 with noise of 0.25 and a few outliers beyond 1 and beyond 8 (F32), or its int8 quantisation: made once."""
    if symbol_type not in _STREAMS:
        rng = np.random.default_rng(20)
        x = (np.where(rng.random(2 * N_STREAM) < 0.5, -0.4, 0.4) + rng.normal(0.0, 0.25, 2 * N_STREAM)).astype(np.float32)
        x[rng.integers(0, len(x), 200)] *= np.float32(30.0)
        if symbol_type == sp.I8:
            x = np.clip(x * 127.0, -128, 127).astype(np.int8)
        x.setflags(write=False)
        _STREAMS[symbol_type] = x
    return _STREAMS[symbol_type][:n]


def up(torch, a, lead=0):
    """The array's bytes in device memory behind `lead` bytes of padding: (the tensor, the pointer to the bytes)."""
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    t = torch.from_numpy(np.concatenate([np.zeros(lead, np.uint8), raw])).to("cuda:0")
    return t, t.data_ptr() + lead


def device_push(xa, torch, mon, a, lead=0, cap=None):
    """One push_device of the array -> (rows, summary); nothing is written behind the rows."""
    n = len(a)
    rows = mon.rows(n)
    cap = rows if cap is None else cap
    t_in, p_in = up(torch, a, lead)
    t_rows = torch.full((64 * (cap + 1),), 0x5A, dtype=torch.uint8, device="cuda:0")
    t_sum = torch.full((32,), 0x5A, dtype=torch.uint8, device="cuda:0")
    mon.push_device(p_in, n, t_rows.data_ptr(), cap, t_sum.data_ptr())
    torch.cuda.synchronize()
    raw = t_rows.cpu().numpy()
    assert (raw[64 * rows:] == 0x5A).all()
    return raw[:64 * rows].view(xa.MONITOR_BLOCK_DTYPE).copy(), t_sum.cpu().numpy().view(xa.MONITOR_SUMMARY_DTYPE)[0].copy()


def same(a, b):
    return a.dtype.itemsize == b.dtype.itemsize and np.array_equal(np.atleast_1d(a).view(np.uint8), np.atleast_1d(b).view(np.uint8))


def check_push(xa, torch, mon, ref, a, lead=0):
    rows, summary = device_push(xa, torch, mon, a, lead)
    want_rows, want_summary = sp.push_fast(ref, a)
    assert len(rows) == len(want_rows) and same(rows, want_rows), (len(a), lead)
    assert same(summary, want_summary), (len(a), lead, summary, want_summary)
    return rows


def check_state(mon, ref):
    got, want = mon.state(), ref.state()
    for name in got.dtype.names:
        assert np.array_equal(got[name], want[name]), (name, got[name], want[name])
    assert same(got, want)


# ---- sizes, types, blocks, pointer offsets ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("symbol_type", (sp.F32, sp.I8))
def test_pushes_equal_the_specification(xa, torch, symbol_type, block):
    """Calls of 0 .. 100 003 symbols one behind the other on one handle, from every pointer offset: the open block, the last
    sign and the histogram carry on."""
    assert xa.MONITOR_BLOCK_DTYPE == sp.BLOCK_DTYPE and xa.MONITOR_STATE_DTYPE == sp.STATE_DTYPE and xa.MONITOR_SUMMARY_DTYPE == sp.SUMMARY_DTYPE
    x = stream(symbol_type)
    sizes = (0, 1, 63, 64, 65, block - 1, block, block + 1, 3 * block + 17, N_STREAM)
    mon, ref = xa.LinkMonitor(block, symbol_type), sp.Monitor(block, symbol_type)
    start = 0
    for lead in LEADS[symbol_type]:
        for n in sizes:
            lo = start % 977                                # the cuts fall differently in every round
            assert mon.rows(n) == ref.rows(n)
            check_push(xa, torch, mon, ref, x[lo:lo + n] if lo + n <= len(x) else x[:n], lead)
            start += n + 131
        check_state(mon, ref)
    mon.close()


def test_a_push_beyond_the_workgroup_grid(xa, torch):
    """Blocks of 2048 take a workgroup per piece on a grid of at most 2048: 37 symbols are open, then one push of
    2048 * (2 * 2048 + 3) - 17 symbols is 4100 pieces (the head of 2011, 4098 whole blocks, a tail of 20), so workgroups 0 to 3
    take three pieces and the others two, each trip through both barriers and the shared partials."""
    block = 2048
    n = block * (2 * 2048 + 3) - 17
    x = np.resize(stream(sp.F32), 37 + n)
    mon, ref = xa.LinkMonitor(block, sp.F32), sp.Monitor(block, sp.F32)
    check_push(xa, torch, mon, ref, x[:37], 0)
    assert sp.piece_count(37, n, block) == 2 * 2048 + 4 and sp.pieces_for(37, n, block)[-1] == (n - 20, n)
    rows = check_push(xa, torch, mon, ref, x[37:], 4)
    assert len(rows) == 2 * 2048 + 3
    check_state(mon, ref)
    mon.close()


# ---- constructed values ----------------------------------------------------------------------------------------------------------
def constructed_f32():
    tiny = np.array([1], np.uint32).view(np.float32)[0]                    # the smallest denormal
    v = [np.nan, np.inf, -np.inf, 0.0, -0.0, 4095 / 512, -4095 / 512, 4095.5 / 512, -4095.5 / 512, 8.0, -8.0, tiny, -tiny,
         1.0, -1.0, 513 / 512, -513 / 512, 0.4, -0.4, 3.4e38, -3.4e38, 4094.5 / 512, -4094.5 / 512]
    for k in (0, 1, 2, 3, 510, 511, 512, 4093, 4094):                       # ties: even and odd k, both signs
        v += [(k + 0.5) / 512, -(k + 0.5) / 512]
    return np.array(v, np.float32)


@pytest.mark.parametrize("lead", (0, 4))
def test_constructed_float_values(xa, torch, lead):
    v = constructed_f32()
    x = np.concatenate([v, stream(sp.F32, 192 - 2 * len(v)), v[::-1]])
    assert len(x) == 192 and len(v) < 64
    mon, ref = xa.LinkMonitor(64), sp.Monitor(64)
    rows = check_push(xa, torch, mon, ref, x, lead)
    check_state(mon, ref)
    # the first block by hand: NaN is bad and q = 0; +-inf, +-4095.5/512, +-8, +-3.4e38 and the ties at 4095.5 clamp
    first = x[:64]
    assert rows[0]["bad"] == 1 and rows[0]["clamped"] == int(np.sum(np.abs(first[~np.isnan(first)].astype(np.float64)) * 512 >= 4095.5))
    loop = sp.Monitor(64)
    want, _ = loop.push(x)
    assert same(rows, want)
    mon.close()


def in_front(values, follow, period, at):
    """`follow` everywhere but at period * j + at, where values[j] stands: every value with `follow` on both sides."""
    x = np.full(period * (len(values) + 1), follow, values.dtype)
    x[at:period * len(values):period] = values
    return x


def each_value_in_front(xa, torch, symbol_type, values, follow, lead, turn):
    """Block 64.  The sign in front of a lane's first symbol is taken from the symbol before it (the device has a function of
    its own for that, apart from the one that takes a symbol in), and from the state in front of a call's first.  Every value
    stands in front of a 16-byte group's first symbol (at every place of a group, so wherever `lead` puts the groups), in
    front of a block's first, and at the end of a call whose successor begins with `follow`."""
    per = 4 if symbol_type == sp.F32 else 16
    mon, ref = xa.LinkMonitor(64, symbol_type), sp.Monitor(64, symbol_type)
    for at in range(per):
        check_push(xa, torch, mon, ref, in_front(values, follow, per, at), lead)
    x = in_front(values, follow, 64, 63 - int(ref.st["open"]["n"]))          # the open symbols shift the blocks
    check_push(xa, torch, mon, ref, x, lead)
    for j, v in enumerate(values):
        check_push(xa, torch, mon, ref, np.array([follow] * (1 + (j + turn) % 5) + [v], values.dtype), lead)
    check_push(xa, torch, mon, ref, np.array([follow], values.dtype), lead)
    check_state(mon, ref)
    mon.close()


@pytest.mark.parametrize("follow", (0.3, -0.3))
def test_every_constructed_float_value_in_front_of_a_group_a_block_and_a_call(xa, torch, follow):
    v = constructed_f32()
    # from the specification alone: for some of them the sign of the lattice value is not the sign of the float
    q = sp.lattice(v, sp.F32)[0]
    assert int(np.sum((q < 0) != (v < 0))) >= 2 and int(np.sum((q < 0) != np.signbit(v))) >= 3
    for turn in range(4):
        each_value_in_front(xa, torch, sp.F32, np.roll(v, turn), np.float32(follow), 4 * turn, turn)


@pytest.mark.parametrize("follow", (40, -40))
def test_every_int8_edge_value_in_front_of_a_group_a_block_and_a_call(xa, torch, follow):
    v = np.array([-128, -1, 0, 1, 127], np.int8)
    for turn, lead in enumerate(LEADS[sp.I8]):
        each_value_in_front(xa, torch, sp.I8, np.roll(v, turn), np.int8(follow), lead, turn)


def test_s4_next_to_two_to_the_63(xa, torch):
    n = 32768
    mon, ref = xa.LinkMonitor(n), sp.Monitor(n)
    rows = check_push(xa, torch, mon, ref, np.full(n + 5, 4095 / 512, np.float32), 12)
    assert int(rows[0]["s4"]) == 4095 ** 4 * n and 0.99 * 2 ** 63 < int(rows[0]["s4"]) < 2 ** 63
    assert int(rows[0]["s2"]) == 4095 ** 2 * n and int(rows[0]["s1"]) == int(rows[0]["sum"]) == 4095 * n and rows[0]["sat"] == n
    assert rows[0]["clamped"] == 0 and rows[0]["flips"] == 0 and rows[0]["neg"] == 0
    check_state(mon, ref)
    assert int(mon.state()["hist"][255]) == n + 5
    # the same at the other end
    rows = check_push(xa, torch, mon, ref, np.full(2 * n - 5, -9.0, np.float32), 4)
    assert int(rows[1]["s4"]) == 4095 ** 4 * n and int(rows[1]["sum"]) == -4095 * n and rows[1]["clamped"] == n and rows[1]["neg"] == n
    assert rows[0]["flips"] == 1 and rows[1]["flips"] == 0
    check_state(mon, ref)
    mon.close()


def test_int8_all_minus_128_and_alternating_signs(xa, torch):
    mon, ref = xa.LinkMonitor(64, sp.I8), sp.Monitor(64, sp.I8)
    rows = check_push(xa, torch, mon, ref, np.full(130, -128, np.int8), 3)
    assert rows[0]["sat"] == 64 and int(rows[0]["sum"]) == -512 * 64 and int(rows[0]["s2"]) == 512 * 512 * 64 and rows[0]["neg"] == 64
    assert int(mon.state()["hist"][(4096 - 512) >> 5]) == 130
    mon.close()
    for symbol_type, block in ((sp.F32, 64), (sp.I8, 64), (sp.F32, 16384), (sp.I8, 16384)):
        alt = np.where(np.arange(2 * block + 7) % 2 == 0, 1, -1)
        a = (alt * 0.3).astype(np.float32) if symbol_type == sp.F32 else (alt * 40).astype(np.int8)
        mon, ref = xa.LinkMonitor(block, symbol_type), sp.Monitor(block, symbol_type)
        rows = check_push(xa, torch, mon, ref, a, 0)
        assert rows[0]["flips"] == block - 1 and rows[1]["flips"] == block       # the second block's first counts against the first's last
        rows = check_push(xa, torch, mon, ref, a[1:], 0)                          # -1 behind +1: the carry-over counts
        assert rows[0]["flips"] == block and int(mon.state()["open"]["n"]) == 13
        rows = check_push(xa, torch, mon, ref, a[2:], 0)                          # +1 behind +1: it does not
        assert rows[0]["flips"] == block - 1 and int(mon.state()["open"]["n"]) == 18
        check_state(mon, ref)
        mon.close()


@pytest.mark.parametrize("symbol_type", (sp.F32, sp.I8))
def test_a_sign_change_at_a_block_boundary_and_at_a_call_boundary(xa, torch, symbol_type):
    block = 16384
    one = np.float32(0.25) if symbol_type == sp.F32 else np.int8(30)
    a = np.full(3 * block, one)
    a[block:] = -one                            # the only change: between the last symbol of block 0 and the first of block 1
    mon, ref = xa.LinkMonitor(block, symbol_type), sp.Monitor(block, symbol_type)
    rows = check_push(xa, torch, mon, ref, a, 4)
    assert [int(r["flips"]) for r in rows] == [0, 1, 0] and [int(r["neg"]) for r in rows] == [0, block, block]
    # the same change between two calls, in the middle of a block and at its end
    for cut in (block // 2 + 3, block):
        mon.reset()
        ref.reset()
        b = np.concatenate([np.full(cut, one), np.full(2 * block - cut, -one)])
        first = check_push(xa, torch, mon, ref, b[:cut], 0)
        second = check_push(xa, torch, mon, ref, b[cut:], 0)
        both = np.concatenate([first, second])
        assert [int(r["flips"]) for r in both] == ([1, 0] if cut < block else [0, 1])
        check_state(mon, ref)
    mon.close()


# ---- a stream and its pieces, reset, two handles, a refused call --------------------------------------------------------------------
@pytest.mark.parametrize("symbol_type", (sp.F32, sp.I8))
def test_a_stream_cut_at_random_equals_one_call(xa, torch, symbol_type):
    x = stream(symbol_type, 100000)
    for block in (64, 16384):
        whole, ref = xa.LinkMonitor(block, symbol_type), sp.Monitor(block, symbol_type)
        rows_whole = check_push(xa, torch, whole, ref, x, 0)
        rng = np.random.default_rng(block + symbol_type)
        cuts = np.sort(np.concatenate([rng.integers(0, len(x), 23), [0, 0, 5000, 5000, len(x), len(x)]]))
        cut, cut_ref = xa.LinkMonitor(block, symbol_type), sp.Monitor(block, symbol_type)
        got = [check_push(xa, torch, cut, cut_ref, x[lo:hi], int(rng.integers(0, 4)) * (4 if symbol_type == sp.F32 else 5))
               for lo, hi in zip(cuts[:-1], cuts[1:])]
        assert same(np.concatenate(got), rows_whole)
        a, b = whole.state(), cut.state()
        assert int(a["calls"]) == 1 and int(b["calls"]) == len(cuts) - 1
        b["calls"] = a["calls"]
        assert same(a, b)
        # reset between streams: the second stream reads as on a fresh handle
        cut.reset()
        cut_ref.reset()
        st = cut.state()
        assert not np.atleast_1d(st).view(np.uint8).any()
        assert same(check_push(xa, torch, cut, cut_ref, x, 0), rows_whole) and same(cut.state(), whole.state())
        whole.close()
        cut.close()


def test_two_handles_at_once(xa, torch):
    x, y = stream(sp.F32), stream(sp.I8)
    a, ra = xa.LinkMonitor(64, sp.F32), sp.Monitor(64, sp.F32)
    b, rb = xa.LinkMonitor(16384, sp.I8), sp.Monitor(16384, sp.I8)
    for lo, hi in ((0, 1000), (1000, 1001), (1001, 40000), (40000, 100003)):
        check_push(xa, torch, a, ra, x[lo:hi], 4)
        check_push(xa, torch, b, rb, y[lo:hi], 1)
    check_state(a, ra)
    check_state(b, rb)
    a.close()
    b.close()


def test_a_refused_call_leaves_the_state_untouched(xa, torch):
    x = stream(sp.F32)
    mon, ref = xa.LinkMonitor(64), sp.Monitor(64)
    check_push(xa, torch, mon, ref, x[:100], 0)
    before = mon.state()
    assert mon.rows(1060) == 17
    with pytest.raises(xa.XritError) as ei:
        device_push(xa, torch, mon, x[100:1160], 0, cap=16)
    assert ei.value.code == -5 and "17 blocks" in str(ei.value)
    with pytest.raises(xa.XritError) as ei:
        mon.push_device(4096, (1 << 30) + 1, 4096, 1 << 30)          # refused for its size before a pointer is looked at
    assert ei.value.code == -1
    assert same(mon.state(), before) and mon.rows(1060) == 17
    check_push(xa, torch, mon, ref, x[100:1160], 0)
    check_state(mon, ref)
    mon.close()


# ---- behind the chain, behind the quantiser ---------------------------------------------------------------------------------------------
def chain_run(xa, torch, d_x, n, sync_each):
    """the chain -> the F32 monitor -> the quantiser -> the I8 monitor on one stream: (soft, bytes, rows, rows8, the states)."""
    dev = torch.device("cuda:0")
    cap = 80000
    dem = xa.Demodulator(xa.Demodulator.config("lrit", 1.25e6, 1, device=0))
    mon, mon8 = xa.LinkMonitor(4096, sp.F32), xa.LinkMonitor(4096, sp.I8)
    d_soft = torch.zeros(cap, dtype=torch.float32, device=dev)
    d_q = torch.zeros(cap, dtype=torch.int8, device=dev)
    d_rows = torch.zeros(64 * 32, dtype=torch.uint8, device=dev)
    d_rows8 = torch.zeros(64 * 32, dtype=torch.uint8, device=dev)
    d_sum = torch.zeros(64, dtype=torch.uint8, device=dev)
    s = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    ns = dem.process_device(d_x.data_ptr(), n, d_soft.data_ptr(), cap, stream=s.cuda_stream)
    if sync_each:
        s.synchronize()
    mon.push_device(d_soft.data_ptr(), ns, d_rows.data_ptr(), 32, d_sum.data_ptr(), stream=s.cuda_stream)
    if sync_each:
        s.synchronize()
    xa.quantize_i8_device(d_soft.data_ptr(), d_q.data_ptr(), ns, stream=s.cuda_stream)
    if sync_each:
        s.synchronize()
    mon8.push_device(d_q.data_ptr(), ns, d_rows8.data_ptr(), 32, d_sum.data_ptr() + 32, stream=s.cuda_stream)
    s.synchronize()
    out = (d_soft.cpu().numpy()[:ns].copy(), d_q.cpu().numpy()[:ns].copy(), d_rows.cpu().numpy().view(xa.MONITOR_BLOCK_DTYPE)[:ns // 4096].copy(),
           d_rows8.cpu().numpy().view(xa.MONITOR_BLOCK_DTYPE)[:ns // 4096].copy(), d_sum.cpu().numpy().view(xa.MONITOR_SUMMARY_DTYPE).copy(),
           mon.state(), mon8.state())
    mon.close()
    mon8.close()
    dem.close()
    return out


def test_behind_the_chain_and_the_quantiser_on_one_stream(xa, torch):
    import synth
    n = 250000
    x = synth.generate(synth.SynthParams(fs_in=1.25e6, esn0_db=8.0), n)
    d_x = torch.from_numpy(x.view(np.float32).copy()).to("cuda:0")
    soft, q8, rows, rows8, sums, st, st8 = chain_run(xa, torch, d_x, n, False)
    soft_s, q8_s, rows_s, rows8_s, sums_s, st_s, st8_s = chain_run(xa, torch, d_x, n, True)
    assert same(soft, soft_s) and same(q8, q8_s) and same(rows, rows_s) and same(rows8, rows8_s) and same(sums, sums_s)
    assert same(st, st_s) and same(st8, st8_s)
    # the rows are the specification's on the device's own symbols
    ref, ref8 = sp.Monitor(4096, sp.F32), sp.Monitor(4096, sp.I8)
    want, want_sum = sp.push_fast(ref, soft)
    want8, want_sum8 = sp.push_fast(ref8, q8)
    assert len(rows) == len(soft) // 4096 >= 10 and same(rows, want) and same(rows8, want8)
    assert same(sums[0], want_sum) and same(sums[1], want_sum8) and same(st, ref.state()) and same(st8, ref8.state())
    # and they say what the burst was, 8 dB, once the loops have settled.  Not the accuracy test (tests/test_monitor_spec.py has
    # it): 1 dB is six times the estimator's standard deviation over 4096 symbols at 8 dB (0.15 dB on AWGN).  Both symbol types
    # share the level scale to 1 % (508 against 512); the quantiser's truncation adds less than another 1 % at this level
    q = [xa.LinkMonitor.derive(r) for r in rows]
    q_8 = [xa.LinkMonitor.derive(r, sp.I8) for r in rows8]
    print("Es/N0 per block:", " ".join(f"{v['esn0_m2m4_db']:.2f}" for v in q), "| int8:", " ".join(f"{v['esn0_m2m4_db']:.2f}" for v in q_8))
    assert all(abs(v["esn0_m2m4_db"] - 8.0) < 1.0 for v in q[4:])
    assert all(abs(a["level"] / b["level"] - 1.0) < 0.02 for a, b in zip(q[4:], q_8[4:]))


# ---- host forms, the host program ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("symbol_type", (sp.F32, sp.I8))
def test_host_forms_equal_the_device_forms(xa, torch, symbol_type):
    x = stream(symbol_type)
    a, b, ref = xa.LinkMonitor(16384, symbol_type), xa.LinkMonitor(16384, symbol_type), sp.Monitor(16384, symbol_type)
    for lo, hi in ((0, 0), (0, 20000), (20000, 20001), (20001, 100003)):
        got = a.push(x[lo:hi])
        assert got.dtype == xa.MONITOR_BLOCK_DTYPE and same(got, check_push(xa, torch, b, ref, x[lo:hi], 0))
    assert same(a.state(), b.state())
    # too little room: XRIT_E_CAPACITY, the rows that were needed, nothing changed
    import ctypes as C
    rows = np.zeros(1, xa.MONITOR_BLOCK_DTYPE)
    need = C.c_size_t(0)
    piece = np.ascontiguousarray(x[:40000])
    rc = xa.lib().xrit_monitor_push(a._h, piece.ctypes.data_as(C.c_void_p), len(piece), rows.ctypes.data_as(C.c_void_p), 1, C.byref(need))
    assert rc == -5 and need.value == a.rows(len(piece)) == 2 and same(a.state(), b.state())
    a.reset()
    assert not np.atleast_1d(a.state()).view(np.uint8).any()
    a.close()
    b.close()


def test_host_program_writes_the_specification_s_csv(xa, torch, tmp_path):
    """xrit_demod_host --monitor on a small capture: the CSV is the specification run on the program's own soft symbols (the
    library's chain on the same blocks, held to the program's int8 output), line for line."""
    import synth
    n, call, block = 300000, 65536, 4096
    x = synth.generate(synth.SynthParams(fs_in=1.25e6, esn0_db=6.0), n)
    capture, out, csv = tmp_path / "burst.cf32", tmp_path / "symbols.s8", tmp_path / "monitor.csv"
    x.tofile(capture)
    host_bin = os.path.join(ROOT, "xritdemod_amd", "bin", "xrit_demod_host")
    base = [host_bin, "--input", str(capture), "--format", "cf32", "--mode", "lrit", "--sample-rate", "1250000", "--block", str(call), "--sink", f"file:{out}"]
    r = subprocess.run(base + ["--monitor", str(csv), "--monitor-block", str(block)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    dem = xa.Demodulator(xa.Demodulator.config("lrit", 1.25e6, 1, device=0))
    soft = [dem.process(x[lo:lo + call]) for lo in range(0, n, call)]
    sent = np.fromfile(out, np.int8)
    assert np.array_equal(sent, dem.quantize_i8(np.concatenate(soft)))
    dem.close()
    ref = sp.Monitor(block)
    lines = ["first,n,level,dc,esn0_m2m4_db,esn0_snv_db,flip_rate,sat_rate,flags"]
    esn0, sat, symbols = [], 0, 0
    for piece in soft:
        for row in sp.push_fast(ref, piece)[0]:
            q = sp.derive(row, sp.F32)
            lines.append("%d,%d,%.6f,%.6f,%.3f,%.3f,%.6f,%.6f,%d" % (row["first"], row["n"], q["level"], q["dc"], q["esn0_m2m4_db"], q["esn0_snv_db"],
                                                                   q["flip_rate"], q["sat_rate"], q["flags"]))
            esn0.append(float(q["esn0_m2m4_db"]))
            sat += int(row["sat"])
            symbols += int(row["n"])
    assert len(lines) - 1 == sum(len(s) for s in soft) // block >= 15
    assert open(csv).read() == "\n".join(lines) + "\n"
    median = sorted(esn0)[len(esn0) // 2]
    low = sum(v < median - 3.0 for v in esn0)
    want = f"monitor: {len(esn0)} blocks, median Es/N0 {median:.2f} dB, {low} blocks more than 3 dB under it, {100.0 * sat / symbols:.4f} % of the symbols saturate int8"
    assert want in r.stderr, r.stderr
    # without --monitor: the same symbols, and stderr without the line
    out.unlink()
    plain = subprocess.run(base, capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0 and "monitor" not in plain.stderr
    assert plain.stderr == r.stderr.replace(want + "\n", "")
    assert np.array_equal(np.fromfile(out, np.int8), sent)
