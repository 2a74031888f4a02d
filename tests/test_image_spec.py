"""CPU tier: the image stage's specification (tests/image_spec.py) against itself -- however a stream is cut into calls,
the rows placed by (vcid, apid, key_serial, row) are the source images; the state inside and behind an image."""
import numpy as np
import pytest

import file_spec as fs
import image_spec as isp
import rice_spec as rs

KEYS = [(0, 10), (0, 11), (7, 10), (63, 2047)]


def run(stream_parts):
    """Both specifications over the calls -> (Rows, image state, outputs per call)."""
    fst, ist, rows, outs = fs.State(), isp.State(), isp.Rows(), []
    for part in stream_parts:
        data, pieces, files, _ = isp.run_files(fst, part)
        out = isp.process(ist, data, pieces, files)
        rows.add(out[0], out[1], files)
        outs.append((files, out))
    return rows, ist, outs


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_every_cutting_gives_the_source_images(seed):
    rng = np.random.default_rng(seed)
    stream, images = isp.random_stream(rng, 8, KEYS, n_other=5, max_cols=150, max_rows=7)
    whole, st_whole, _ = run([stream])
    for k in (1, 3, 20):
        rows, st, outs = run(list(fs.cut_calls(rng, stream, k)))
        assert rows.rows.keys() == whole.rows.keys()
        for key, (x, status) in rows.rows.items():
            assert status == whole.rows[key][1] and np.array_equal(x, whole.rows[key][0]), key
        for c in isp.COUNTERS:
            assert getattr(st, c) == getattr(st_whole, c), c
        assert {k_: v.as_tuple() for k_, v in st.keys.items()} == {k_: v.as_tuple() for k_, v in st_whole.keys.items()}
        # the lines of one call are in piece order and packed back to back, padded to a multiple of 4
        for files, (data, lines, ifiles, summary) in outs:
            assert (np.diff(lines["piece"].astype(np.int64)) > 0).all()
            assert (lines["offset"] % 4 == 0).all() and len(data) == summary["bytes"] == int(ifiles["length"].sum())
            assert len(ifiles) == len(files) and summary["images"] == int(ifiles["rice"].sum())
    assert st_whole.images_begun == st_whole.images_completed == len(images) and st_whole.images_aborted == 0
    for (v, a, serial), img in images.items():
        x, status = whole.image(v, a, serial)
        assert not status.any() and np.array_equal(x, img), (v, a, serial)
    assert len(whole.rows) == sum(len(i) for i in images.values()) == st_whole.total_lines and st_whole.total_faults == 0


def test_state_inside_an_image_and_after_an_abort():
    rng = np.random.default_rng(4)
    img, data, cuts = isp.image_file(rng, 10, 32, 70, 9)
    spoiled = lambda r, line: rs.truncate(r, line)
    img2, data2, cuts2 = isp.image_file(rng, 8, 8, 20, 6, spoil=spoiled)
    stream = isp.stream_of(rng, [((3, 5), data, cuts, 8190), ((3, 5), data2, cuts2, 8190)], seq_start=16380)
    assert len(stream) == 10 + 7
    # the first call ends inside the first image: header and four lines
    rows, st, outs = run([stream[:5]])
    k = st.keys[(3, 5)]
    assert k.as_tuple() == (1, 0, 4, 0) and (st.images_begun, st.images_completed, st.total_lines) == (1, 0, 4)
    ifile = outs[0][1][2][0]
    assert (int(ifile["rice"]), int(ifile["first_row"]), int(ifile["n_lines"]), int(ifile["lines_total"])) == (1, 0, 4, 4)
    # the rest of it, and the second image without its last packet: open, with its truncated lines counted as faults
    rows, st, outs = run([stream[:5], stream[5:16]])
    files, (_, lines, ifiles, summary) = outs[1]
    assert [int(x) for x in ifiles["first_row"]] == [4, 0] and [int(x) for x in ifiles["lines_total"]] == [9, 5]
    k = st.keys[(3, 5)]
    assert k.open == 1 and k.key_serial == 1 and k.lines == 5 and k.faults == int(lines["status"][5:].astype(bool).sum()) > 0
    assert st.images_completed == 1 and np.array_equal(rows.image(3, 5, 0)[0], img)
    # a packet lost inside the second image: the next packet of the key aborts it -- the bare ABORTED record closes the state
    rows, st, outs = run([stream[:5], stream[5:14], stream[15:]])
    files, (_, lines, ifiles, summary) = outs[2]
    assert len(files) == 1 and int(files[0]["flags"]) == fs.ABORTED and int(files[0]["n_pieces"]) == 0
    assert int(ifiles[0]["rice"]) == 1 and int(ifiles[0]["n_lines"]) == 0 and int(ifiles[0]["first_row"]) == 3 == int(ifiles[0]["lines_total"])
    assert st.keys[(3, 5)].open == 0 and st.images_aborted == 1 and summary["lines"] == 0
    # a reset of the image stage inside an image: its later lines are nobody's
    fst, ist = fs.State(), isp.State()
    isp.process(ist, *isp.run_files(fst, stream[:5])[:3])
    ist = isp.State()
    out = isp.process(ist, *isp.run_files(fst, stream[5:])[:3])
    assert [int(x) for x in out[2]["rice"]] == [0, 1] and out[3]["lines"] == 6


def test_a_tiled_call_is_well_formed_and_every_copy_is_the_base():
    stream, cut, images = isp.tiling_base()
    fst, base_state = fs.State(), isp.State()
    base = [isp.run_files(fst, stream[:cut]), isp.run_files(fst, stream[cut:])]
    base_out, base_key = [], []
    for b in base:
        base_out.append(isp.process(base_state, *b[:3]))
        base_key.append(base_state.keys[(0, 0)].as_tuple())
    assert [int(x) for x in base_out[0][2]["rice"]] == [0, 1, 1] and [int(x) for x in base_out[1][2]["rice"]] == [1]
    assert base_key == [(1, 2, 1, 1), (0, 2, 3, 1)] and base_state.total_faults == 2
    copies = 3
    ist, rows = isp.State(), isp.Rows()
    for b, want, key_after in zip(base, base_out, base_key):
        data, pieces, files, summ = call = isp.tile_call(b, copies)
        assert (summ["files"], summ["pieces"], summ["bytes"]) == (len(files), len(pieces), len(data)) == \
               (copies * len(b[2]), copies * len(b[1]), copies * len(b[0]))
        # ordered by key; every record's pieces contiguous, its own, inside the pieces; every piece inside the bytes
        keys = files["vcid"].astype(np.int64) * 2048 + files["apid"]
        assert (np.diff(keys) >= 0).all() and sorted(set(keys)) == list(range(copies))
        assert np.array_equal(files["first_piece"][1:], (files["first_piece"] + files["n_pieces"])[:-1])
        assert int(files["first_piece"][0]) == 0 and int(files["first_piece"][-1]) + int(files["n_pieces"][-1]) == len(pieces)
        assert np.array_equal(pieces["file"], np.repeat(np.arange(len(files)), files["n_pieces"]))
        assert np.array_equal(pieces["offset"][1:], (pieces["offset"] + pieces["length"])[:-1]) and int(pieces["offset"][0]) == 0
        assert int(pieces["offset"][-1]) + int(pieces["length"][-1]) == len(data)
        for r in files:
            mine = pieces[int(r["first_piece"]):int(r["first_piece"]) + int(r["n_pieces"])]
            assert (mine["vcid"] == r["vcid"]).all() and (mine["apid"] == r["apid"]).all()
            assert int(mine["length"].sum()) == int(r["length"]) and (not len(mine) or int(mine[0]["offset"]) == int(r["offset"]))
        out = isp.process(ist, data, pieces, files)
        rows.add(out[0], out[1], files)
        # every copy: the base's outputs, moved; the base's state on its key
        nl, nb = len(want[1]), len(want[0])
        assert np.array_equal(out[0], np.tile(want[0], copies)) and len(out[1]) == copies * nl
        for c in range(copies):
            mine = out[1][c * nl:(c + 1) * nl]
            for f in ("length", "row", "samples", "bits", "status"):
                assert np.array_equal(mine[f], want[1][f]), f
            assert np.array_equal(mine["offset"], want[1]["offset"] + np.uint64(c * nb))
            assert np.array_equal(mine["file"], want[1]["file"] + c * len(b[2])) and np.array_equal(mine["piece"], want[1]["piece"] + c * len(b[1]))
        assert all(ist.keys[(0, c)].as_tuple() == key_after for c in range(copies))
        # the head of a call: exactly its records' pieces and bytes
        for n in (0, 1, len(b[2]), len(files) - 1, len(files)):
            hd, hp, hf, hs = isp.head_of_call(call, n)
            assert (hs["files"], hs["pieces"], hs["bytes"]) == (len(hf), len(hp), len(hd)) == \
                   (n, int(files["n_pieces"][:n].sum()), int(files["length"][:n].sum()))
            assert hf.tobytes() == files[:n].tobytes() and (not n or int(hp["file"].max()) == n - 1)
    for c in isp.COUNTERS:
        assert getattr(ist, c) == copies * getattr(base_state, c), c
    for c in range(copies):
        for serial, img in images.items():
            x, status = rows.image(0, c, serial)
            assert np.array_equal(x[status == 0], img[status == 0]) and list(status) == ([0, 1] if serial == 1 else [1, 0, 0])
    # a copy beyond apid 2047 goes to the next channel
    files = isp.tile_call(base[0], 2050)[2]
    assert (int(files[-1]["vcid"]), int(files[-1]["apid"])) == (1, 1) and (int(files[2047 * 3]["vcid"]), int(files[2047 * 3]["apid"])) == (0, 2047)


def test_the_link_rule_and_the_padding():
    rng = np.random.default_rng(5)
    img, data, cuts = isp.image_file(rng, 8, 8, 5, 3)
    plain = fs.lrit_file(bytes(40), image=(8, 5, 3, 0))                     # an image, not compressed
    items = [((1, 1), data, cuts, 8190), ((1, 2), data, None, 8190),       # the same file with data in its first packet
             ((1, 3), plain, None, 8190)]
    fst, ist = fs.State(), isp.State()
    data_, pieces, files, _ = isp.run_files(fst, isp.stream_of(rng, items))
    out, lines, ifiles, summary = isp.process(ist, data_, pieces, files)
    assert [int(x) for x in ifiles["rice"]] == [1, 0, 0] and ifiles[1:].tobytes() == bytes(96)
    assert summary["lines"] == 3 and summary["bytes"] == 24 and [int(x) for x in lines["length"]] == [5, 5, 5]
    assert [int(x) for x in lines["offset"]] == [0, 8, 16] and not out.reshape(3, 8)[:, 5:].any()
    assert np.array_equal(out.reshape(3, 8)[:, :5], img)
