"""GPU tier: the canvas stage (xrit_canvas_*, ImageCanvas) against the specification of tests/canvas_spec.py -- per-record
outputs, slot table, segment tables, key states, counters and every byte of every slot's pixels, after every call: mixed
images in one call, the stream cut into small calls, every reason, an aborted segment, a release under an open file,
refused calls, reset and two handles, the device path behind packets, files and images on one stream, calls tiled over
4 097 keys, faulted lines; and xrit_demod_host --canvas from IQ to .pgm files.  Those streams hold images of at most
64 x 48 pixels for slots of 16 KiB.
At real sizes, from calls built by hand (canvas_cases.direct_call) and one real-size stream: every copy path of the place
kernel past a wave's first 64 units (lines of 1051 and 5568 bytes from every residue mod 16 to every residue), the image
bytes 4, 8 and 12 bytes off a 16-byte boundary in device memory, a line of 131070 bytes into a slot filled to its last
byte and TOO_LARGE on either side of that, records of 135 lines in one call and cut in two, images of 64 and of 63
segments (bit 63, the upper lanes of the rectangle test, DUPLICATE and OVERLAP there), lines at and behind the end of
the image bytes, lines longer than their segment; 2784 x 140 at 10 bit and 1051 x 130 through the stages in front.
Every comparison is exact."""
import functools

import numpy as np
import pytest

import canvas_cases as cc
import canvas_spec as cs
import file_spec as fs
import image_spec as isp
import packet_spec as ps

pytestmark = pytest.mark.gpu


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


def record(dtype, summ, overflow=0):
    """A summary record of that dtype from the specification's dict."""
    s = np.zeros(1, dtype)
    for k, v in summ.items():
        s[0][k] = v
    s[0]["overflow"] = overflow
    return s


def inputs(xa, files_out, images_out, files_overflow=0, images_overflow=0):
    return (files_out[:3] + (record(xa.FILES_SUMMARY_DTYPE, files_out[3], files_overflow),),
            images_out[:3] + (record(xa.IMAGES_SUMMARY_DTYPE, images_out[3], images_overflow),))


def same(got, want):
    cfiles, slots, summary = got
    wfiles, wslots, wsum = want
    for k, w in wsum.items():
        assert int(summary[k]) == w, k
    assert int(summary["overflow"]) == 0
    assert cfiles.tobytes() == wfiles.tobytes()
    assert slots.tobytes() == wslots.tobytes()


def pixels(torch, cv):
    """Every byte of every slot."""
    t = torch.zeros(cv.slots * cv.slot_bytes, dtype=torch.uint8, device="cuda:0")
    for s in range(cv.slots):
        cv.read_device(s, t.data_ptr() + s * cv.slot_bytes, cv.slot_bytes)
    torch.cuda.synchronize()
    return t.cpu().numpy().reshape(cv.slots, cv.slot_bytes)


def same_state(torch, cv, st, keys=None):
    s = cv.stats()
    for c in cs.COUNTERS:
        assert int(s[c]) == getattr(st, c), c
    for i in range(st.n_slots):
        assert cv.segments(i).tobytes() == st.segments[i].tobytes(), i
    for v, a in (st.keys if keys is None else keys):
        assert cv.key(v, a).tobytes() == st.key(v, a).tobytes(), (v, a)
    assert np.array_equal(pixels(torch, cv), st.pixels)


def drive(xa, torch, run, keys=None):
    """The device over the calls of a canvas_cases.Run, everything compared after every call -> the handle."""
    cv = xa.ImageCanvas(run.slots, run.slot_bytes)
    for i, (files_out, images_out, want, st) in enumerate(run.calls):
        for s in run.actions.get(i, ()):
            cv.release(s)
        same(cv.process(*inputs(xa, files_out, images_out)), want)
        same_state(torch, cv, st, keys)
    return cv


def test_mixed_images_in_one_call(xa, torch):
    stream, images = cc.mixed_stream()
    run = cc.Run([stream], slots=6)
    out, slots, summ = run.calls[0][2]
    # from the specification alone: the case holds what it is for
    assert summ["canvases_completed"] == 5 and {int(b) for b in slots["bits"][:5]} == {8, 10, 12}
    widths = {int(s["start_column"]) * cs.width_of(int(slots[int(s["slot"])]["bits"])) % 4 for s in out if s["reason"] == cs.PLACED}
    assert widths == {0, 1, 2} and 1 in slots["max_column"]
    cv = drive(xa, torch, run)
    for i in range(5):
        info, img = cv.image(i)
        v, bits, want = images[int(info["image_id"])]
        assert int(info["complete"]) == 1 and (int(info["vcid"]), int(info["bits"])) == (v, bits) and np.array_equal(img, want)
    assert bytes(cv.read(0)[0]["name"]).rstrip(b"\0") == b"IMG A/8 bit.lrit"
    cv.close()


@pytest.mark.parametrize("seed", [1, 2])
def test_cut_into_small_calls(xa, torch, seed):
    stream, images = cc.mixed_stream()
    run = cc.Run(list(fs.cut_calls(np.random.default_rng(seed), stream, 4)), slots=6)
    assert len(run.calls) > len(stream) // 4
    cv = drive(xa, torch, run)
    done = 0
    for i in range(6):
        info, img = cv.image(i)
        if info["in_use"]:
            assert int(info["complete"]) == 1 and np.array_equal(img, images[int(info["image_id"])][2])
            done += 1
    assert done == 5
    cv.close()


def test_every_reason(xa, torch):
    stream, want, img = cc.reasons_stream()
    run = cc.Run([stream], slots=8)
    assert [int(r) for r in run.calls[0][2][0]["reason"]] == want and run.calls[0][2][2]["lines_clipped"] == 2
    cv = drive(xa, torch, run)
    assert np.array_equal(cv.image(int(run.calls[0][2][0]["slot"][10]))[1], img)
    cv.close()
    run = cc.Run([stream[:len(stream) // 2], stream[len(stream) // 2:]], slots=8)
    assert run.calls[1][2][2]["no_placement"] >= 2
    drive(xa, torch, run).close()
    run = cc.Run([cc.no_slot_stream()], slots=2)
    assert run.calls[0][2][2]["no_slot"] == 1
    drive(xa, torch, run).close()


def test_aborted_segment_keeps_its_rows_and_is_not_accepted_again(xa, torch):
    stream, img, kept = cc.aborted_stream()
    run = cc.Run([stream[:7], stream[7:]])
    out, slots, summ = run.calls[1][2]
    assert int(slots[0]["aborted_mask"]) == 2 and not slots[0]["complete"] and summ["duplicate"] == 1 and summ["segments_aborted"] == 1
    cv = drive(xa, torch, run)
    got = cv.image(0)[1]
    assert np.array_equal(got[:4 + kept], img[:4 + kept]) and not got[4 + kept:8].any() and np.array_equal(got[8:], img[8:])
    cv.close()


def test_release_while_a_file_is_open(xa, torch):
    first, second, new = cc.release_streams()
    run = cc.Run([first, second], actions={1: [0]})
    assert sorted(int(r) for r in run.calls[1][2][0]["reason"]) == [cs.PLACED, cs.NO_PLACEMENT, cs.NO_PLACEMENT]
    cv = drive(xa, torch, run)
    info, img = cv.image(0)
    want = np.zeros((8, 16), np.uint8)
    want[1:4, 3:13] = new
    assert int(info["generation"]) == 1 and int(info["image_id"]) == 41 and np.array_equal(img, want)
    cv.close()


def test_refused_calls_reset_and_two_handles(xa, torch):
    stream, _ = cc.mixed_stream()
    half = len(stream) // 2
    run = cc.Run([stream[:half], stream[half:]], slots=6)
    (f1, i1, w1, st1), (f2, i2, w2, st2) = run.calls
    cv, other = xa.ImageCanvas(6, cc.SLOT_BYTES), xa.ImageCanvas(6, cc.SLOT_BYTES)
    same(cv.process(*inputs(xa, f1, i1)), w1)
    # refused through the host buffers: each summary's overflow, a count beyond each bound
    cut = lambda t, k: t[:k] + (t[k][:-1],) + t[k + 1:]
    for fin, iin in (inputs(xa, f2, i2, files_overflow=1), inputs(xa, f2, i2, images_overflow=1),
                     (cut(inputs(xa, f2, i2)[0], 1), inputs(xa, f2, i2)[1]), (inputs(xa, f2, i2)[0], cut(inputs(xa, f2, i2)[1], 1))):
        with pytest.raises(xa.XritError) as ei:
            cv.process(fin, iin)
        assert ei.value.code == -1 and int(ei.value.partial[0]["overflow"]) == 2
        assert bytes(ei.value.partial[0].tobytes()[40:160]) == cv.stats().tobytes()
        same_state(torch, cv, st1)
    # ... and through device pointers: only the summary is written
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
    fin, iin = inputs(xa, f2, i2, images_overflow=1)
    d = [up(a) for a in fin + iin]
    d_cf, d_slots, d_sum = (torch.full((n,), 0xA5, dtype=torch.uint8, device=dev) for n in (len(f2[2]) * 32, 6 * 136, 168))
    cv.process_device(d[0].data_ptr(), len(f2[0]), d[1].data_ptr(), len(f2[1]), d[2].data_ptr(), len(f2[2]), d[3].data_ptr(),
                      d[4].data_ptr(), len(i2[0]), d[5].data_ptr(), len(i2[1]), d[6].data_ptr(), d[7].data_ptr(), d_cf.data_ptr(),
                      d_slots.data_ptr(), d_sum.data_ptr())
    torch.cuda.synchronize()
    assert int(d_sum.cpu().numpy().view(xa.CANVAS_SUMMARY_DTYPE)[0]["overflow"]) == 2
    assert (d_cf.cpu().numpy() == 0xA5).all() and (d_slots.cpu().numpy() == 0xA5).all()
    same_state(torch, cv, st1)
    # the call that is not refused goes on from the unchanged state; a second handle meanwhile runs the whole stream
    whole = cc.Run([stream], slots=6)
    same(other.process(*inputs(xa, *whole.calls[0][:2])), whole.calls[0][2])
    same(cv.process(*inputs(xa, f2, i2)), w2)
    same_state(torch, cv, st2)
    same_state(torch, other, whole.state)
    cv.reset()
    fresh = cs.State(6, cc.SLOT_BYTES)
    same_state(torch, cv, fresh, keys=list(st2.keys))
    same(cv.process(*inputs(xa, *whole.calls[0][:2])), whole.calls[0][2])
    same_state(torch, cv, whole.state)
    cv.close()
    other.close()


def test_device_path_behind_packets_files_and_images_on_one_stream(xa, torch):
    rng = np.random.default_rng(68)
    stream, images = cc.mixed_stream(69)
    by_vc = {}
    for v, p, *_ in stream:
        by_vc.setdefault(v, []).append(p)
    dummies = lambda count: [fs.space_packet(99, i, 3, rng.integers(0, 256, 800, dtype=np.uint8).tobytes()) for i in range(count)]
    rows = {v: ps.rows_of(ps.build_stream(v, dummies(1) + pk + dummies(2), rng, fill=0.0, idle=0.0)) for v, pk in by_vc.items()}
    parts = [ps.group({v: r[:len(r) // 2] for v, r in rows.items()}), ps.group({v: r[len(r) // 2:] for v, r in rows.items()})]
    dev = torch.device("cuda:0")
    z = lambda nbytes: torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    pa, fa, im, cv = xa.PacketAssembler(), xa.FileAssembler(), xa.ImageDecoder(), xa.ImageCanvas(6, cc.SLOT_BYTES)
    bufs = []
    for vcdu, off in parts:
        n = int(off[64])
        cap = 4 * n                                             # bounds four times the counts
        mb, mp = xa.packets_max_bytes(cap), 16 * cap + 64
        sizes = dict(pbytes=mb, desc=mp * 32, pko=65 * 4, psum=72, fbytes=mb, pieces=mp * 32, frecs=2 * mp * 80, fsum=104, out=mp * 256,
                     lines=mp * 32, ifiles=2 * mp * 48, isum=80, cfiles=2 * mp * 32, slots=6 * 136, csum=168)
        b = {k: z(v) for k, v in sizes.items()}
        b["vcdu"] = torch.cat([torch.from_numpy(vcdu.reshape(-1).copy()).to(dev), z((cap - n) * 892)])
        b["off"] = torch.from_numpy(off.view(np.uint8).copy()).to(dev)
        bufs.append((cap, mb, mp, b))
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        for cap, mb, mp, b in bufs:
            q = {k: t.data_ptr() for k, t in b.items()}
            pa.process_device(q["vcdu"], q["off"], cap, q["pbytes"], mb, q["desc"], mp, q["pko"], q["psum"], stream=s.cuda_stream)
            fa.process_device(q["pbytes"], mb, q["desc"], q["pko"], mp, q["fbytes"], mb, q["pieces"], mp, q["frecs"], 2 * mp, q["fsum"],
                              stream=s.cuda_stream)
            im.process_device(q["fbytes"], mb, q["pieces"], mp, q["frecs"], 2 * mp, q["fsum"], q["out"], mp * 256, q["lines"], mp,
                              q["ifiles"], q["isum"], stream=s.cuda_stream)
            cv.process_device(q["fbytes"], mb, q["pieces"], mp, q["frecs"], 2 * mp, q["fsum"], q["out"], mp * 256, q["lines"], mp,
                              q["ifiles"], q["isum"], q["cfiles"], q["slots"], q["csum"], stream=s.cuda_stream)
    s.synchronize()                                             # the only one of this test's own
    # the host-buffer path, stage by stage
    h_pa, h_fa, h_im, h_cv = xa.PacketAssembler(), xa.FileAssembler(), xa.ImageDecoder(), xa.ImageCanvas(6, cc.SLOT_BYTES)
    for (vcdu, off), (cap, mb, mp, b) in zip(parts, bufs):
        pdata, pdesc, pko = h_pa.process(vcdu, off)[:3]
        files_out = h_fa.process(pdata, pdesc, pko)
        images_out = h_im.process(*files_out)
        want = h_cv.process(files_out, images_out)
        nf = int(files_out[3]["files"])
        assert b["csum"].cpu().numpy().tobytes() == want[2].tobytes() and int(want[2]["overflow"]) == 0
        assert b["cfiles"].cpu().numpy()[:nf * 32].tobytes() == want[0].tobytes() and not b["cfiles"].cpu().numpy()[nf * 32:].any()
        assert b["slots"].cpu().numpy().tobytes() == want[1].tobytes()
    assert int(want[2]["canvases_completed"]) == 5 and cv.stats().tobytes() == h_cv.stats().tobytes()
    assert np.array_equal(pixels(torch, cv), pixels(torch, h_cv))
    for i in range(5):
        info, img = cv.image(i)
        assert np.array_equal(img, images[int(info["image_id"])][2])
    for x in (pa, fa, im, cv, h_pa, h_fa, h_im, h_cv):
        x.close()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


@functools.lru_cache(maxsize=None)
def tiled():
    """image_spec.tiling_base's two calls -- a file that is no image, an 8-bit image, a 12-bit image left open; then its
    rest --, each over 4 097 keys, and the specification's images calls on them: 8 194 images without record 128, each a
    canvas of its own; shared, never changed."""
    stream, cut, _ = isp.tiling_base()
    fst, ist = fs.State(), isp.State()
    calls = []
    for part in (stream[:cut], stream[cut:]):
        files_out = isp.tile_call(isp.run_files(fst, part), 4097)
        calls.append((files_out, isp.process(ist, *files_out[:3])))
    return calls


def test_calls_tiled_over_4097_keys(xa, torch):
    st = cs.State(64, cc.SLOT_BYTES)
    cv = xa.ImageCanvas(64, cc.SLOT_BYTES)
    keys = [(0, 0), (0, 31), (0, 32), (0, 2047), (1, 0), (2, 0)]
    for i, (files_out, images_out) in enumerate(tiled()):
        assert len(files_out[2]) == (3 if i == 0 else 1) * 4097
        want = cs.process(st, files_out, images_out)
        if i == 0:
            assert want[2]["no_slot"] == 2 * 4097 - 64 and want[2]["canvases_begun"] == 64 and want[2]["completed"] == 32
        else:
            assert want[2]["no_placement"] == 4097 - 32 and want[2]["completed"] == 32 and want[1]["complete"].all()
        same(cv.process(*inputs(xa, files_out, images_out)), want)
        same_state(torch, cv, st, keys)
    cv.close()


def test_faulted_lines_are_placed_as_the_image_stage_wrote_them(xa, torch):
    stream = cc.faulted_stream()
    fst, ist = fs.State(), isp.State()
    data, pieces, files, summ = isp.run_files(fst, stream)
    cut = int(pieces[-1]["offset"]) + 1                          # the last piece lies outside the bytes: its line has status 2
    files_out = (data[:cut], pieces, files, summ)
    images_out = isp.process(ist, *files_out[:3])
    assert [int(x) for x in images_out[1]["status"]] == [0, 1, 0, 2]
    st = cs.State(2, cc.SLOT_BYTES)
    want = cs.process(st, files_out, images_out)
    assert (int(want[0][0]["lines_placed"]), int(want[0][0]["faults"])) == (4, 2) and int(want[1][0]["faults"]) == 2
    assert int(want[1][0]["complete"]) == 1 and st.image(0)[1].any() and not st.image(0)[3].any()
    cv = xa.ImageCanvas(2, cc.SLOT_BYTES)
    same(cv.process(*inputs(xa, files_out, images_out)), want)
    same_state(torch, cv, st)
    cv.close()


# ---- calls built by hand (canvas_cases.direct_call): what the stages in front never vary ---------------------------------
@functools.lru_cache(maxsize=None)
def copy_run():
    """canvas_cases.copy_path_call and the specification's run of it: shared, never changed."""
    call, _ = cc.copy_path_call()
    return call, cc.Run([call], slots=64, slot_bytes=cc.COPY_SLOT_BYTES, direct=True)


def device_call(xa, torch, cv, files_out, images_out, pad=0):
    """One process_device on the call's arrays, the image bytes uploaded behind `pad` bytes -> what process returns."""
    fin, iin = inputs(xa, files_out, images_out)
    dev = torch.device("cuda:0")
    up = lambda a, lead=0: torch.from_numpy(np.concatenate([np.zeros(lead, np.uint8), np.ascontiguousarray(a).view(np.uint8).reshape(-1)])).to(dev)
    d_bytes, d_pieces, d_files, d_fsum = (up(a) for a in fin)
    d_img, d_lines, d_ifiles, d_isum = up(iin[0], pad), up(iin[1]), up(iin[2]), up(iin[3])
    assert d_img.data_ptr() % 16 == 0
    nf = len(fin[2])
    d_cf, d_slots, d_sum = (torch.zeros(n, dtype=torch.uint8, device=dev) for n in (nf * 32, cv.slots * 136, 168))
    cv.process_device(d_bytes.data_ptr(), len(fin[0]), d_pieces.data_ptr(), len(fin[1]), d_files.data_ptr(), nf, d_fsum.data_ptr(),
                      d_img.data_ptr() + pad, len(iin[0]), d_lines.data_ptr(), len(iin[1]), d_ifiles.data_ptr(), d_isum.data_ptr(),
                      d_cf.data_ptr(), d_slots.data_ptr(), d_sum.data_ptr())
    torch.cuda.synchronize()
    return (d_cf.cpu().numpy().view(xa.CANVAS_FILE_DTYPE), d_slots.cpu().numpy().view(xa.CANVAS_SLOT_DTYPE),
            d_sum.cpu().numpy().view(xa.CANVAS_SUMMARY_DTYPE)[0])


def test_every_copy_path_on_its_second_trip(xa, torch):
    """Lines of 1051 bytes (16 * 65 + 4 * 2 + 3) and of 5568 (2784 samples of two bytes) from every residue mod 16 of the
    image bytes the stages in front never produce (they pad to 4) to rows whose first bytes fall on every residue a pitch
    of 12 mod 16 gives: the 16-byte loop with its dword and byte tails, dwords alone, dword loads with byte stores, and
    bytes, each past its wave's first 64."""
    call, run = copy_run()
    took = cc.copy_paths(call)                                  # from the call's own numbers, before the device is touched
    assert took["16"] >= 4 and took["16, 4, 1"] >= 2 and took["4"] >= 32 and took["4 to bytes"] >= 32 and took["bytes"] >= 32, took
    assert run.calls[0][2][2]["call_lines_placed"] == 256 and run.state.slots["complete"].all()
    cv = drive(xa, torch, run)
    info, img = cv.image(63)
    assert int(info["bits"]) == 10 and np.array_equal(img, run.state.image(63))
    cv.close()


@pytest.mark.parametrize("pad", (4, 8, 12))
def test_image_bytes_4_8_and_12_bytes_off_a_16_byte_boundary(xa, torch, pad):
    """The library asks 4-byte alignment of the image bytes, and the place kernel picks its path from the addresses: the
    same call from device memory with the image bytes moved, so that other lines take the 16-byte path."""
    call, run = copy_run()
    files_out, images_out, want, st = run.calls[0]
    moved, there = cc.copy_paths(call, image_base=pad), cc.copy_paths(call)
    assert moved != there and all(n >= 2 for n in moved.values()), moved
    cv = xa.ImageCanvas(64, cc.COPY_SLOT_BYTES)
    same(device_call(xa, torch, cv, files_out, images_out, pad), want)
    same_state(torch, cv, st)
    cv.close()


def test_the_widest_line_fills_a_slot_to_its_last_byte(xa, torch):
    """65535 columns of 16 bits: lines of 131070 bytes, 128 trips of the 16-byte loop, in a slot of exactly pitch * max_row
    bytes; the same image with a third row declared is TOO_LARGE there, and both are in a slot 16 bytes smaller."""
    call, slot_bytes = cc.widest_line_calls()
    run = cc.Run([call], slots=2, slot_bytes=slot_bytes, direct=True)
    assert [int(r) for r in run.calls[0][2][0]["reason"]] == [cs.PLACED, cs.TOO_LARGE]
    assert int(run.state.slots[0]["pitch"]) * 2 == slot_bytes and run.state.pixels[0, slot_bytes - 3] != 0
    cv = drive(xa, torch, run)
    info, img = cv.image(0)
    assert img.shape == (2, 65535) and np.array_equal(img, run.state.image(0)) and img[1, 65534] != 0
    cv.close()
    run = cc.Run([call], slots=2, slot_bytes=slot_bytes - 16, direct=True)
    assert [int(r) for r in run.calls[0][2][0]["reason"]] == [cs.TOO_LARGE] * 2 and not run.state.slots["in_use"].any()
    drive(xa, torch, run).close()


def test_records_of_more_lines_than_a_wave_has_lanes(xa, torch):
    """135 lines in one record, permuted, some faulted, some beyond the segment's 129 declared lines: every trip of the commit
    kernel's loop adds to placed, clipped and faults.  Then the same file cut after 65 lines into a record that begins and
    one that only continues and ends."""
    trips = cc.tall_counts(cc.tall_entries())
    assert len(trips) == 3 and all(n > 0 for t in trips for n in t)
    one, cut = cc.tall_calls()
    run = cc.Run([one], direct=True)
    o = run.calls[0][2][0][0]
    assert [int(o["lines_placed"]), int(o["lines_clipped"]), int(o["faults"])] == [sum(t[i] for t in trips) for i in range(3)]
    drive(xa, torch, run).close()
    run = cc.Run(cut, direct=True)
    assert [int(c[2][0][0]["lines_placed"]) for c in run.calls] == [63, 66] and int(run.state.slots[0]["complete"]) == 1
    assert int(run.calls[1][0][2][0]["flags"]) == fs.ENDS
    drive(xa, torch, run).close()


def test_images_of_64_and_63_segments(xa, torch):
    """Bit 63 of the masks, lanes 32 to 63 of the rectangle test, `complete` at 64 segments and at 63
    (canvas_cases.sixty_four_segment_calls)."""
    calls, (full, late), part = cc.sixty_four_segment_calls()
    run = cc.Run(calls, direct=True)
    assert [int(s["done_mask"]) for s in run.state.slots] == [2 ** 64 - 1, 2 ** 63 - 1, 2 ** 64 - 1, 1 << 63 | 1 << 32 | 4]
    assert [int(s["complete"]) for s in run.calls[2][3].slots] == [1, 1, 0, 0] and [int(s["complete"]) for s in run.state.slots] == [1, 1, 1, 0]
    assert [int(r) for r in run.calls[4][2][0]["reason"]] == [cs.DUPLICATE]
    assert [int(r) for r in run.calls[5][2][0]["reason"]] == [cs.PLACED, cs.PLACED, cs.OVERLAP, cs.OVERLAP, cs.PLACED]
    cv = drive(xa, torch, run)
    assert int(cv.segments(0)["begun"].sum()) == 64 and int(cv.segments(1)["begun"].sum()) == 63
    for slot, want in ((0, full), (1, part), (2, late)):
        assert np.array_equal(cv.image(slot)[1], want)
    cv.close()


def test_lines_at_the_end_of_the_image_bytes_and_lines_too_long(xa, torch):
    """canvas_line_dst's guard on inputs the stages in front never emit: a line that ends on the last image byte, one that
    ends one behind it, an empty one at the end, an offset of 2^63; lines longer than their segment is wide."""
    run = cc.Run(cc.guard_calls(), direct=True)
    o = run.calls[1][2][0][0]
    assert (int(o["lines_placed"]), int(o["lines_clipped"])) == (2, 2) and len(run.calls[1][1][0]) == 64
    assert [int(x) for x in run.calls[1][1][1]["offset"]] == [56, 57, 64, 1 << 63]
    o = run.calls[2][2][0][0]
    assert (int(o["lines_placed"]), int(o["lines_clipped"])) == (3, 1) and run.state.image(1)[1:, :4].all()
    drive(xa, torch, run).close()


def test_real_line_and_segment_sizes_through_the_stages(xa, torch):
    """A 10-bit image of 2784 x 140 in two segments on two keys and an 8-bit image of 1051 x 130 cut 2 x 2, through the
    specifications of the packet, file and image stages, the stream cut into two calls."""
    stream, images = cc.real_size_stream()
    half = len(stream) // 2
    run = cc.Run([stream[:half], stream[half:]], slots=2, slot_bytes=cc.REAL_SLOT_BYTES)
    lines = np.concatenate([c[1][1] for c in run.calls])
    assert {int(x) % 16 for x in lines["offset"]} == {0, 4, 8, 12} and {int(x) for x in lines["length"]} >= {5568, 523, 528}
    assert max(int(x) for c in run.calls for x in c[1][2]["n_lines"]) > 64
    assert run.state.slots["complete"].all() and run.calls[1][2][2]["lines_placed"] == 140 + 2 * 130
    cv = drive(xa, torch, run)
    for slot in range(2):
        info, img = cv.image(slot)
        assert np.array_equal(img, images[int(info["image_id"])])
    assert bytes(cv.read(int(np.flatnonzero(run.state.slots["image_id"] == 500)[0]))[0]["name"]).rstrip(b"\0") == b"full width, 10 bit"
    cv.close()


def host_capture(tmp_path, by_vc, seed):
    """IQ samples of the packets per channel, as tests/test_gpu_files.py makes them for the host program -> path."""
    import ccsds
    import synth
    rng = np.random.default_rng(seed)
    dummies = lambda count, seq: [fs.space_packet(99, seq + i, 3, rng.integers(0, 256, 600, dtype=np.uint8).tobytes()) for i in range(count)]
    rows = {v: ps.rows_of(ps.build_stream(v, dummies(7, 0) + pk + dummies(6, 7), rng, fill=0.0, idle=0.0)) for v, pk in by_vc.items()}
    sent, k = [], 0
    while any(k < len(r) for r in rows.values()):
        sent += [rows[v][k] for v in sorted(rows) if k < len(rows[v])]
        k += 1
    cadus = np.stack([ccsds.cadu_from_block(ps.block_of(r)) for r in sent])
    sym = ccsds.coded_symbols(cadus, amplitude=1).astype(np.float64)
    p = synth.SynthParams(fs_in=1.25e6, seed=seed, esn0_db=12.0)
    synth.generate(p, int((len(sym) + 64) * p.sps_in), symbols=sym).tofile(tmp_path / "iq.cf32")
    return tmp_path / "iq.cf32"


def test_host_program_canvas(xa, tmp_path):
    """End to end from IQ: an 8-bit image of two segments on two apids with an annotation, a 10-bit image of one segment
    without, and an image whose second segment never comes -> <name>.pgm, vc..._img..._....pgm, ....partial.pgm; the
    .lrit and .img files are there as without --canvas."""
    import os
    import subprocess
    rng = np.random.default_rng(70)
    a, b, c = cs.samples(rng, 8, 16, 64, 12), cs.samples(rng, 10, 32, 33, 5), cs.samples(rng, 8, 8, 16, 4)
    items = cs.split_image(rng, a, 8, 16, 21, [(5, 40), (5, 41)], [7], name=b"GOES test/full disk.lrit")
    items += cs.split_image(rng, b, 10, 32, 22, [(5, 42)], [])
    items += cs.split_image(rng, np.concatenate([c, c]), 8, 8, 23, [(5, 43)], [4])[:1]
    by_vc = {5: [p for _, p, _ in isp.stream_of(rng, items)]}
    iq = host_capture(tmp_path, by_vc, 70)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    host_bin = os.path.join(root, "xritdemod_amd", "bin", "xrit_demod_host")
    out = tmp_path / "files"
    r = subprocess.run([host_bin, "--input", str(iq), "--mode", "lrit", "--sample-rate", "1250000", "--sink", "null", "--block", "200000",
                        "--files", str(out), "--files-decompress", "--canvas", "--canvas-slots", "4", "--canvas-mib", "1"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    names = set(os.listdir(out))
    assert (out / "GOES_test_full_disk.lrit.pgm").read_bytes() == b"P5\n64 12\n255\n" + a.astype(np.uint8).tobytes()
    plain = [nm for nm in names if nm.startswith("vc5_img22_") and nm.endswith(".pgm")]
    assert len(plain) == 1 and (out / plain[0]).read_bytes() == b"P5\n33 5\n1023\n" + b.astype(">u2").tobytes()
    partial = [nm for nm in names if nm.endswith(".partial.pgm")]
    assert len(partial) == 1 and partial[0].startswith("vc5_img23_")
    assert (out / partial[0]).read_bytes() == b"P5\n16 8\n255\n" + c.astype(np.uint8).tobytes() + bytes(16 * 4)
    assert len([nm for nm in names if nm.endswith(".pgm")]) == 3 and len([nm for nm in names if nm.endswith(".img")]) == 4
    assert (out / "vc5_apid42_0.img").read_bytes() == b.astype("<u2").tobytes()
    line = [ln for ln in r.stderr.splitlines() if ln.startswith("canvas:")]
    assert len(line) == 1 and "3 images begun, 3 written (1 of them partial), 21 lines placed, 0 clipped, 0 segment files refused" in line[0]
