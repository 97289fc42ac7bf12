"""The JPEG ingest without a GPU: the host reader (read_jpeg_raw / read_jpeg in host/uvol_host.cpp) against the NumPy restatement of the decoding
rule, uvol_idct_jpeg_batch_dev (csrc/jpeg_ingest.hip) through the host emulation of the kernels (tests/hipemu), and `uvolenc` / the `basisu`
shim linked against the emulation library.  The checks are in tests/jpeg_cases.py; tests/test_gpu_jpeg.py runs the device ones on the MI355X."""
import os
import subprocess
import pytest
import jpeg_cases as JC
import material_cases as MC
from conftest import ROOT

PKG = os.path.join(ROOT, "universal-volumetric_amd")


@pytest.fixture(scope="module")
def host():
    subprocess.check_call(["make", "-s", "-C", PKG, "libuvolhost.so"])
    return JC.hostlib()


@pytest.fixture()
def emu(hipemu_lib):
    import uvol
    cd = uvol.Codec(lib_path=hipemu_lib)
    yield cd
    cd.close()


@pytest.fixture(scope="module")
def emu_bins():
    subprocess.check_call(["make", "-s", "-C", PKG, "hipemu-bins"])
    return os.path.join(ROOT, "tests", "hipemu", "bin")


def test_jpeg_host_reader_equals_the_rule(host):
    """1. uvolh_jpeg_coeffs = the plain-Python Huffman decode, uvolh_jpeg_decode_rgba = the NumPy rule, bit for bit, on every accepted fixture."""
    JC.run_host(host)


def test_jpeg_rule_is_close_to_libjpeg():
    """4. The rule (equal to the device by the bit-exactness tests) against Pillow's decode of the same files (golden/jpeg/expected.npz)."""
    worst, low = JC.measure_libjpeg()
    print("largest channel difference %d, lowest PSNR %.2f dB" % (worst, low))
    assert worst <= JC.LIBJPEG_MAX_DIFF and low >= JC.LIBJPEG_MIN_PSNR, (worst, low)


def test_jpeg_host_refusals(host):
    """6. Each refusal fixture gives its status and a message that names the feature."""
    JC.run_host_refusals(host)


def test_hipemu_jpeg_fixtures_bit_exact(emu, host):
    JC.run_device_fixtures(emu, MC.HostMem(), host)


def test_hipemu_jpeg_batch_of_five_both_slots(emu):
    JC.run_device_batch(emu, MC.HostMem())


def test_hipemu_jpeg_inputs_in_host_alloc_memory(emu, host, hipemu_lib):
    import uvol
    arena = uvol.PinnedArena(1 << 20, lib_path=hipemu_lib)
    try:
        JC.run_device_fixtures(emu, MC.HostMem(), host, arena=arena)
        JC.run_device_batch(emu, MC.HostMem(), arena=arena)
    finally:
        arena.close()


def test_hipemu_jpeg_arithmetic_edges(emu):
    JC.run_arithmetic_edges(emu, MC.HostMem())


def test_hipemu_jpeg_into_the_encoder(oracle, emu):
    JC.run_into_encoder(oracle, emu, MC.HostMem())


def test_hipemu_jpeg_into_the_uastc_encoder(oracle, hipemu_lib):
    import uvol
    cu = uvol.Codec(lib_path=hipemu_lib, uastc=1)
    try:
        JC.run_into_encoder(oracle, cu, MC.HostMem(), uastc=True)
    finally:
        cu.close()


def test_hipemu_jpeg_bad_arguments_and_trim(emu):
    import numpy as np
    import uvol
    mem = MC.HostMem()
    ptrs, want = JC.run_bad_arguments(emu, uvol.UvolError)
    assert np.array_equal(JC.read_layers(mem, ptrs, 16, 16)[0], want)
    emu.trim()                                                 # uvol_trim gives the slots back; the next call allocates again
    P, want = JC.reference("c420_17x9")
    ptrs = emu.idct_jpeg_batch_dev([P.coef], [P.qt], P.w, P.h, 3, 2, 2, slot=1)
    assert np.array_equal(JC.read_layers(mem, ptrs, P.w, P.h)[0], want)


@pytest.mark.parametrize("name", sorted(JC.DRIVER_RUNS))
def test_uvolenc_hipemu_jpeg_sequence(oracle, emu_bins, tmp_path, name):
    """7. device path, --host-png-unfilter, and a mixed PNG / JPEG sequence."""
    JC.run_driver(oracle, os.path.join(emu_bins, "uvolenc"), str(tmp_path), name)


def test_uvolenc_hipemu_jpeg_corrupt_frame_fails_its_segment(oracle, emu_bins, tmp_path):
    JC.run_driver_corrupt_frame(oracle, os.path.join(emu_bins, "uvolenc"), str(tmp_path))


def test_basisu_shim_hipemu_reads_jpeg(oracle, emu_bins, tmp_path):
    JC.run_basisu_shim(oracle, os.path.join(emu_bins, "basisu"), str(tmp_path))


FUZZ_MAIN = r"""
// every accepted fixture through read_jpeg_raw and read_jpeg; three of them also at every truncation length and with every byte of the first
// 700 replaced by 00, FF and D9: each case returns success or an error (the sanitizers report anything else)
#include "uvol_host.hpp"
#include <cstdio>
#include <cstring>
int main(int argc, char **argv) {
  long cases = 0, ok = 0;
  for (int a = 1; a < argc; a++) {
    const bool mutate = argv[a][0] == '+'; const char *path = argv[a] + (mutate ? 1 : 0);
    std::vector<uint8_t> d; if (!uvolh::read_file(path, d)) { std::fprintf(stderr, "cannot read %s\n", path); return 2; }
    uvolh::JpegRaw J; uvolh::Image im; std::string e;
    if (uvolh::read_jpeg_raw(path, J, e) != 1 || !uvolh::read_jpeg(path, im, e) || im.rgba.size() != (size_t)J.w * J.h * 4) { std::fprintf(stderr, "%s: %s\n", path, e.c_str()); return 3; }
    if (!mutate) continue;
    std::vector<uint8_t> rgba;
    auto run = [&](const uint8_t *p, size_t n) {
      uvolh::JpegRaw R; std::string err; const int r = uvolh::read_jpeg_raw_mem(p, n, "case", R, err); cases++;
      if (r == 1) { ok++; rgba.resize((size_t)R.w * R.h * 4); uvolh::jpeg_decode_rgba(R, rgba.data()); }
      else if (err.empty()) { std::fprintf(stderr, "status %d without a message\n", r); std::exit(4); }
    };
    for (size_t n = 0; n < d.size(); n++) { std::vector<uint8_t> t(d.begin(), d.begin() + (long)n); run(t.data(), t.size()); }      // (a copy of its own size: a read past it is a report)
    static const uint8_t repl[3] = { 0x00, 0xff, 0xd9 };
    for (size_t i = 0; i < d.size() && i < 700; i++) for (uint8_t v : repl) { if (d[i] == v) continue; std::vector<uint8_t> t(d); t[i] = v; run(t.data(), t.size()); }
  }
  std::printf("%ld cases, %ld decoded\n", cases, ok);
  return 0;
}
"""


def test_jpeg_parser_survives_hostile_input(tmp_path):
    """8. A stand-alone program built from host/uvol_host.cpp with -fsanitize=address,undefined (it loads no Python and preloads nothing)."""
    src = tmp_path / "jpeg_fuzz.cpp"; src.write_text(FUZZ_MAIN); exe = str(tmp_path / "jpeg_fuzz")
    host = os.path.join(PKG, "host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", host, str(src),
                           os.path.join(host, "uvol_host.cpp"), "-o", exe, "-lz", "-ldl", "-lpthread"])
    mutated = ("c420_17x9", "rstblk_420_33x17", "stuffed_444_24x16")
    args = [("+" if n in mutated else "") + os.path.join(JC.GOLD, n + ".jpg") for n in JC.ACCEPTED + JC.SEQUENCE]
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    print(r.stdout)
