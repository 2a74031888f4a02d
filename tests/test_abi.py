"""CPU tier: the C-ABI library loads, exports every symbol include/xritdemod_amd.h declares, its host-side
designers agree with the oracle, and the compute entry points fail loudly without a HIP device."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "xritdemod_amd.h")


@pytest.fixture(scope="module")
def xa():
    import xritdemod_amd
    if not os.path.exists(xritdemod_amd.lib_path()):
        xritdemod_amd.build()
    xritdemod_amd.lib()
    return xritdemod_amd


def declared_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(xrit_[a-z0-9_]+)\s*\(", src)))


def test_every_declared_symbol_is_exported(xa):
    names = declared_functions()
    assert len(names) >= 35
    out = subprocess.check_output(["nm", "-D", "--defined-only", xa.lib_path()], text=True)
    exported = set(line.split()[-1] for line in out.splitlines() if line.strip())
    missing = [n for n in names if n not in exported]
    assert not missing, missing
    # and the ctypes binding covers all of them
    from xritdemod_amd import _capi
    assert sorted(_capi._SIGNATURES) == names


def test_header_cites_reference_interfaces():
    src = open(HEADER).read()
    for needle in ("demodulator.cpp:443-444", "demodulator.cpp:100-168", "SymbolManager.cpp:43-46",
                   "FrontendDevice.h:11-13", "Parameters.h:34-37"):
        assert needle in src, needle


def test_host_designers_match_oracle(xa, oracle_mod):
    o = oracle_mod
    assert np.array_equal(xa.Filters.RRC(1, 1.25e6, 293883, 0.5, 63), o.rrc_taps(1, 1.25e6, 293883, 0.5, 63))
    assert np.array_equal(xa.Filters.RRC(1, 2.5e6, 927000, 0.3, 63), o.rrc_taps(1, 2.5e6, 927000, 0.3, 63))
    assert np.array_equal(xa.Filters.lowPass(1, 6.25e6, 625e3, 100e3), o.lowpass_taps(1, 6.25e6, 625e3, 100e3))
    assert np.array_equal(xa.Filters.lowPass(1, 40e6, 625e3, 100e3), o.lowpass_taps(1, 40e6, 625e3, 100e3))
    assert np.array_equal(xa.Filters.mmse_table(), o.mmse_table())


def test_config_presets_follow_parameters_h(xa):
    c = xa.Demodulator.config("lrit", 3e6, 2)
    assert (c.symbol_rate, c.rrc_taps, c.decimation) == (293883, 63, 2)
    assert abs(c.rrc_alpha - 0.5) < 1e-7 and abs(c.pll_alpha - 0.0037) < 1e-9      # demodulator.cpp:220 quirk
    assert abs(c.clock_gain_omega - 0.0037 ** 2 / 4) < 1e-12 and c.agc_max_gain == 4000
    h = xa.Demodulator.config("hrit", 2.5e6, 1)
    assert h.symbol_rate == 927000 and abs(h.rrc_alpha - 0.3) < 1e-7


def test_no_silent_cpu_path(xa):
    """Without a HIP device every compute object must refuse to exist (no fallback)."""
    if xa.device_count() > 0:
        pytest.skip("a HIP device is present")
    for make in (lambda: xa.AGC(0.01, 0.5, 1, 4000), lambda: xa.CostasLoop(0.0037),
                 lambda: xa.FirFilter(1, np.ones(3, np.float32)),
                 lambda: xa.ClockRecovery(4.25, 3.4e-6, 0.5, 0.0037, 0.005),
                 lambda: xa.Demodulator(xa.Demodulator.config("lrit"))):
        with pytest.raises(xa.XritError) as ei:
            make()
        assert ei.value.code == -2
        assert "no CPU path" in str(ei.value)


def test_product_package_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "xritdemod_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".h")):
                text = open(os.path.join(dirpath, f), errors="replace").read()
                assert "import oracle" not in text and "xrit_oracle" not in text and "oracle/" not in text, f


HOST_BIN = os.path.join(ROOT, "xritdemod_amd", "bin", "xrit_demod_host")


def test_host_program_builds_and_has_no_cpu_path(xa, tmp_path):
    """The file-source / TCP-sink host loop is plain C++ on the C ABI; without a HIP
    device it must fail loudly instead of demodulating on the CPU."""
    assert os.path.exists(HOST_BIN), "make -C xritdemod_amd/csrc builds it"
    r = subprocess.run([HOST_BIN], capture_output=True, text=True)
    assert r.returncode == 2 and "usage:" in r.stderr
    host = os.path.join(ROOT, "xritdemod_amd", "host")
    pieces = sorted(os.listdir(host))
    assert "xrit_demod_host.cpp" in pieces
    for name in pieces:                          # the boundary is the C ABI only, in every piece of the program
        src = open(os.path.join(host, name)).read()
        assert "hip/hip_runtime" not in src and "<hip/" not in src, name
    if xa.device_count() > 0:
        pytest.skip("a HIP device is present")
    f = tmp_path / "x.cf32"
    np.zeros(2048, np.complex64).tofile(f)
    r = subprocess.run([HOST_BIN, "--input", str(f), "--sink", "null"], capture_output=True, text=True)
    assert r.returncode == 1 and "no CPU path" in r.stderr


def test_integration_md_snippets_compile_against_the_header(tmp_path):
    """INTEGRATION.md shows the code a maintainer of the reference would write; the self-contained snippets (the
    SatHelper-shaped wrapper classes, the decoder's correlator and frame-fix calls) must at least parse against
    include/xritdemod_amd.h."""
    import re
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "INTEGRATION.md")).read()
    blocks = re.findall(r"```cpp\n(.*?)```", text, re.S)
    wrapper = next(b for b in blocks if "namespace XritAmd" in b)
    corr = next(b for b in blocks if "xrit_sync_correlate(" in b)
    fix = next(b for b in blocks if "xrit_sync_fix_frames(" in b)
    group = next(b for b in blocks if "xrit_group_process_slice_device(" in b)
    a = tmp_path / "wrapper.cpp"
    a.write_text('#include <complex>\n#include <vector>\n#include <stdexcept>\n#include "xritdemod_amd.h"\n' + wrapper +
                 "\nint main() { return 0; }\n")
    b = tmp_path / "decoder.cpp"
    b.write_text('#include <cstdint>\n#include <cstddef>\n#include "xritdemod_amd.h"\n#define CODEDFRAMESIZE 16384\n'
                 "#define MINCORRELATIONBITS 46\nstruct V { void decode(const int8_t *, uint8_t *) {} };\n"
                 "void f(uint8_t *codedData, const int8_t *symbols, size_t nSymbols, size_t nFrames, xrit_sync_hit *hits,\n"
                 "       int8_t *frames, uint8_t *valid, uint8_t *decodedData) {\n    V viterbi;\n" + corr +
                 "\n(void)word; (void)pos; (void)corr;\n" + fix + "\n}\nint main() { return 0; }\n")
    c = tmp_path / "group.cpp"
    c.write_text('#include <cstdint>\n#include <cstddef>\n#include "xritdemod_amd.h"\n' + group + "\nint main() { return 0; }\n")
    for src in (a, b, c):
        r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I" + os.path.join(root, "include"), str(src)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def test_shipped_build_has_no_matrix_pipe_code():
    """BASELINE.json's north star: no MFMA on this path.  The f32-MFMA decimator of round 3 (an experiment that lost its
    A/B, profiles/r3_mfma_decimator.txt) is compiled only with make EXTRA=-DXRIT_EXPERIMENTS: the device code of a default
    build of csrc/fir.hip holds no v_mfma instruction, and the library says which build it is."""
    import shutil
    import subprocess
    import tempfile
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "xritdemod_amd", "csrc", "fir.hip")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "fir.s")
        subprocess.check_call([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-S", "--cuda-device-only",
                               "-o", out, src], stderr=subprocess.DEVNULL)
        text = open(out).read()
    assert "fir_decim_kernel" in text and "v_mfma" not in text
    import xritdemod_amd
    assert xritdemod_amd.build_experiments() is False
