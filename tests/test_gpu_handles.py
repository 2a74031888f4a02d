"""GPU tier: what the four stateful back-end handles (FrameDecoder, ChannelDemux, PacketAssembler, FileAssembler) share
-- create, reset, read-back and close around the own stream and the stream of the last call -- at the smallest shapes:
one frame, one row, one packet.  A fresh handle reset and read before any call; a handle closed right after a
host-buffer call and right after a call on a side stream that nobody waited for; a device that does not exist.  Every
comparison is exact."""
import numpy as np
import pytest

import ccsds
import demux_spec as ds
import file_spec as fs
import packet_spec as ps

pytestmark = pytest.mark.gpu

STAGES = ["decoder", "demux", "packets", "files"]


@pytest.fixture(scope="module")
def xa():
    import xritdemod_amd
    xritdemod_amd.lib()
    if xritdemod_amd.device_count() < 1:
        pytest.fail("the -m gpu tier needs a HIP device; the library has no CPU path")
    return xritdemod_amd


def raw(x):
    return np.ascontiguousarray(x).reshape(-1).view(np.uint8)


def same(got, want):
    return len(got) == len(want) and all(np.array_equal(raw(g), raw(w)) for g, w in zip(got, want))


class Decoder:
    """One clean LRIT frame: the specification's result is the CADU and the block that were coded."""

    def __init__(self, xa):
        rng = np.random.default_rng(41)
        self.block = ccsds.make_block(0x8C, 5, 100, rng)[None]
        self.cadu = ccsds.cadu_from_block(self.block[0])[None]
        self.frames = ccsds.coded_symbols(self.cadu).reshape(1, ccsds.FRAME_SYMBOLS).astype(np.int8)
        self.valid = np.ones(1, np.uint8)
        self.make = lambda device=0: xa.FrameDecoder("lrit", device=device)
        self.info_dtype = xa.FRAME_INFO_DTYPE

    def host(self, h):
        return h.decode(self.frames, self.valid)

    def check(self, out):
        cadu, block, info = out
        assert np.array_equal(cadu, self.cadu) and np.array_equal(block, self.block)
        assert (int(info["ok"][0]), int(info["vcid"][0]), int(info["counter"][0]), int(info["viterbi_errors"][0])) == (1, 5, 100, 0)

    def check_start(self, h):
        pass                                        # the carry has no read-back: reset() returning is the check

    def device(self, h, torch, dev, s):
        t = [torch.from_numpy(self.frames.view(np.uint8)).to(dev), torch.from_numpy(self.valid).to(dev)]
        o = [torch.zeros(n, dtype=torch.uint8, device=dev) for n in (1024, 1020, self.info_dtype.itemsize)]
        s.wait_stream(torch.cuda.current_stream(dev))
        h.decode_device(t[0].data_ptr(), t[1].data_ptr(), 1, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), stream=s.cuda_stream)
        return t, lambda: (o[0].cpu().numpy()[None], o[1].cpu().numpy()[None], o[2].cpu().numpy().view(self.info_dtype))


class Demux:
    """One good frame on channel 5."""

    def __init__(self, xa):
        rng = np.random.default_rng(42)
        self.info = np.zeros(1, xa.FRAME_INFO_DTYPE)
        for k, v in (("valid", 1), ("ok", 1), ("viterbi_errors", 83), ("scid", 0x8C), ("vcid", 5), ("counter", 100)):
            self.info[k] = v
        self.info["rs_errors"] = [0, 3, -1, 16]
        self.hits = np.array([[1, 77, 60, 0]], np.uint32)
        self.cadu = np.zeros((1, 1024), np.uint8)
        self.cadu[:, :4] = rng.integers(0, 256, 4)
        self.block = rng.integers(0, 256, (1, 1020), dtype=np.uint8)
        self.make = lambda device=0: xa.ChannelDemux(device=device)
        self.xa = xa

    def args(self):
        return self.hits, self.cadu, self.block, self.info

    def host(self, h):
        return h.process(*self.args())

    def check(self, out):
        want = ds.process(ds.State(), *self.args(), wire=False)[:3]
        assert np.array_equal(out[0], want[0]) and np.array_equal(out[1], want[1]) and out[2].tobytes() == want[2].tobytes()
        assert int(out[1][64]) == 1

    def check_start(self, h):
        s, w = h.stats(), ds.State()
        assert [int(s[k]) for k in ("total_packets", "dropped_packets", "lost_packets", "sum_viterbi_errors", "sum_rs_corrections")] == [0] * 5
        assert s["received"].tolist() == w.received and s["lost"].tolist() == w.lost_vc and s["last_counter"].tolist() == w.last

    def device(self, h, torch, dev, s):
        t = [torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev) for a in self.args()]
        o = [torch.zeros(n, dtype=torch.uint8, device=dev) for n in (892, 65 * 4, 88)]
        s.wait_stream(torch.cuda.current_stream(dev))
        h.process_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), 1, o[0].data_ptr(), o[1].data_ptr(),
                         o[2].data_ptr(), stream=s.cuda_stream)
        return t, lambda: (o[0].cpu().numpy()[None], o[1].cpu().numpy().view(np.uint32), o[2].cpu().numpy().view(self.xa.FRAME_STATS_DTYPE))


class Packets:
    """One row on channel 5 that holds whole packets."""

    def __init__(self, xa):
        rng = np.random.default_rng(43)
        packets = [ps.make_packet(700 + i, i, 60, rng) for i in range(40)]
        self.vcdu, self.off = ps.group({5: ps.build_stream(5, packets, rng, fill=0.0, idle=0.0).rows[:1]})
        assert int(self.off[64]) == 1
        self.make = lambda device=0: xa.PacketAssembler(device=device)
        self.xa = xa

    def host(self, h):
        return h.process(self.vcdu, self.off)

    def check(self, out):
        data, desc, pko, summary = out
        wdata, wdesc, wpko, wsum = ps.process(ps.State(), self.vcdu, self.off)
        assert len(wdesc) >= 1 and np.array_equal(pko, wpko) and desc.tobytes() == wdesc.tobytes() and np.array_equal(data, wdata)
        assert all(int(summary[k]) == w for k, w in wsum.items()) and int(summary["overflow"]) == 0

    def check_start(self, h):
        s, w = h.stats(), ps.State()
        for k in ps.COUNTERS:
            assert [int(x) for x in s["vc_" + k]] == getattr(w, k) and int(s[k]) == 0, k
        assert [int(x) for x in s["last_counter"]] == w.last and not s["pending_bytes"].any()

    def device(self, h, torch, dev, s):
        xa = self.xa
        mb, mp = xa.packets_max_bytes(1), 127 + 64
        t = [torch.from_numpy(self.vcdu.reshape(-1).copy()).to(dev), torch.from_numpy(self.off.view(np.uint8).copy()).to(dev)]
        o = [torch.zeros(n, dtype=torch.uint8, device=dev) for n in (mb, mp * 32, 65 * 4, 72)]
        s.wait_stream(torch.cuda.current_stream(dev))
        h.process_device(t[0].data_ptr(), t[1].data_ptr(), 1, o[0].data_ptr(), mb, o[1].data_ptr(), mp, o[2].data_ptr(), o[3].data_ptr(),
                         stream=s.cuda_stream)

        def read():
            summary = o[3].cpu().numpy().view(xa.PACKETS_SUMMARY_DTYPE)[0]
            return (o[0].cpu().numpy()[:int(summary["bytes"])], o[1].cpu().numpy().view(xa.PACKET_DTYPE)[:int(summary["packets"])],
                    o[2].cpu().numpy().view(np.uint32), summary)
        return t, read


class Files:
    """One packet that is a whole file, on (5, 700)."""

    def __init__(self, xa):
        pkt = fs.packetise(fs.lrit_file(bytes(range(200)), image=(8, 20, 10, 0)), 700, 3, 9)[0]
        assert len(pkt) == 1
        self.args = fs.stage_input([(5, pkt[0])])
        self.make = lambda device=0: xa.FileAssembler(device=device)
        self.xa = xa

    def host(self, h):
        return h.process(*self.args)

    def check(self, out):
        data, pieces, files, summary = out
        wdata, wpieces, wfiles, wsum = fs.process(fs.State(), *self.args)
        assert len(wpieces) == 1 and wsum["files_completed"] == 1
        assert pieces.tobytes() == wpieces.tobytes() and files.tobytes() == wfiles.tobytes() and np.array_equal(data, wdata)
        assert all(int(summary[k]) == w for k, w in wsum.items()) and int(summary["overflow"]) == 0

    def check_start(self, h):
        assert h.stats().tobytes() == bytes(80) and h.key(5, 700).tobytes() == bytes(56)

    def device(self, h, torch, dev, s):
        xa = self.xa
        data, desc, pko = self.args
        t = [torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev) for a in (data, desc, pko)]
        o = [torch.zeros(n, dtype=torch.uint8, device=dev) for n in (len(data), 32, 2 * 80, 104)]
        s.wait_stream(torch.cuda.current_stream(dev))
        h.process_device(t[0].data_ptr(), len(data), t[1].data_ptr(), t[2].data_ptr(), 1, o[0].data_ptr(), len(data), o[1].data_ptr(), 1,
                         o[2].data_ptr(), 2, o[3].data_ptr(), stream=s.cuda_stream)

        def read():
            summary = o[3].cpu().numpy().view(xa.FILES_SUMMARY_DTYPE)[0]
            return (o[0].cpu().numpy()[:int(summary["bytes"])], o[1].cpu().numpy().view(xa.FILE_PIECE_DTYPE)[:int(summary["pieces"])],
                    o[2].cpu().numpy().view(xa.FILE_RECORD_DTYPE)[:int(summary["files"])], summary)
        return t, read


CASES = {"decoder": Decoder, "demux": Demux, "packets": Packets, "files": Files}


@pytest.fixture(scope="module")
def cases(xa):
    return {k: c(xa) for k, c in CASES.items()}


@pytest.mark.parametrize("stage", STAGES)
def test_fresh_handle_reset_read_close(cases, stage):
    c = cases[stage]
    h = c.make()
    h.reset()
    c.check_start(h)
    h.close()


@pytest.mark.parametrize("stage", STAGES)
def test_close_after_a_host_call_and_again_on_a_new_handle(cases, stage):
    c = cases[stage]
    h = c.make()
    first = c.host(h)
    h.close()
    h = c.make()
    second = c.host(h)
    h.close()
    c.check(first)
    assert same(first, second)


@pytest.mark.parametrize("stage", STAGES)
def test_close_right_after_a_call_on_a_side_stream(cases, stage):
    torch = pytest.importorskip("torch")
    c = cases[stage]
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream(device=dev)
    h = c.make()
    keep, read = c.device(h, torch, dev, s)
    h.close()                                       # nobody has waited for s
    torch.cuda.synchronize()
    c.check(read())
    h = c.make()
    c.check(c.host(h))
    h.close()
    del keep


def test_a_device_that_does_not_exist(xa, cases):
    codes = []
    for stage in STAGES:
        with pytest.raises(xa.XritError) as ei:
            cases[stage].make(device=xa.device_count())
        assert "out of range" in str(ei.value), stage
        codes.append(ei.value.code)
    assert codes == [-1] * 4                        # XRIT_E_INVALID from all four
