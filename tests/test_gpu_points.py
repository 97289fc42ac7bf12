"""The render-ready mesh decode (uvol_decode_mesh_batch_points) on a real MI355X, through the C ABI: the checks of tests/points_cases.py
(shared with tests/test_hipemu_points.py) on all 250 recorded files, and one call at the bench's size."""
import os
import numpy as np
import pytest
import material_cases as MC
import points_cases as PC
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture()
def gpu_codec0():
    import uvol
    c = uvol.Codec(device=0, DRACO_COMPRESSION_LEVEL=0)
    yield c
    c.close()


def test_gpu_points_all_recorded_files(oracle):
    """Check 1: all 250 recorded files in one call per layout, bit-exact against the reference, plus the renderer's invariant on every file."""
    import uvol
    cd = uvol.Codec(device=0, max_batch=250)
    try:
        assert PC.run_recorded(oracle, cd, PC.recorded_files()) == 250
    finally:
        cd.close()


def test_gpu_points_attribute_subsets_and_tool_sets(oracle, gpu_codec, gpu_codec0):
    PC.run_subsets(oracle, gpu_codec, gpu_codec0)


def test_gpu_points_ragged_batch_fails_per_frame(oracle, gpu_codec, gpu_codec0):
    PC.run_ragged(oracle, gpu_codec, gpu_codec0)


def test_gpu_points_long_fan_is_refused_alone(oracle, gpu_codec, gpu_codec0):
    PC.run_long_fan(oracle, gpu_codec, gpu_codec0)


def test_gpu_points_memory_forms(oracle, gpu_codec, gpu_codec0):
    """Check 4: outputs in HBM (written in place by the weld kernels), in pageable host memory and in a PinnedArena."""
    PC.run_memory_forms(oracle, gpu_codec, gpu_codec0, MC.HipMem())


def test_gpu_points_round_trip_through_the_encoder(oracle, gpu_codec):
    """Check 5: the welded buffers stay in HBM and go into uvol_encode_mesh_batch_dev with one index stream for all three attributes."""
    PC.run_round_trip(oracle, gpu_codec, MC.HipMem())


def test_gpu_points_existing_decode_untouched(oracle, gpu_codec, gpu_codec0):
    files = [f for _, f in PC.subset_streams(gpu_codec, gpu_codec0)][:5] + [open(os.path.join(GOLDEN, n), "rb").read() for n in ("00000.drc", "00075.drc")]
    PC.run_existing_untouched(oracle, gpu_codec, files)


def test_gpu_points_at_bench_size(oracle):
    """Check 7: ONE call of 256 frames of the bench's shape (about 100 k vertices / 200 k faces; 16 distinct connectivities, each stored 16
    times), interleaved records written straight into HBM.  A seeded sample of 8 frames is compared bit for bit with the reference; of the
    others n_points and the CRC of the index array are compared with the reference's."""
    import synth, uvol
    nd, n = 16, 256
    cd = uvol.Codec(device=0, max_batch=n)
    mem = MC.HipMem()
    try:
        distinct = cd.encode_mesh_batch([MC.plain(m) for m in synth.distinct_meshes(nd, bases=nd)])
        files = [distinct[i % nd] for i in range(n)]
        st, metas, _, ptr = decode_dev_counts(cd, mem, files)
        assert st == [0] * n
        refs = [PC.reference(oracle, f) for f in distinct]
        assert all(r["n_faces"] > 190000 and r["n_points"] > 100000 for r in refs)
        sample = set(int(i) for i in np.random.default_rng(11).choice(n, 8, replace=False))
        for i in range(n):
            r = refs[i % nd]; m = metas[i]
            assert (m.n_faces, m.n_points, m.has_uv, m.has_nrm) == (r["n_faces"], r["n_points"], 1, 1), i
            idx = mem.to_host(ptr[i]["index"], np.uint32, 3 * m.n_faces)
            assert PC.index_crc(idx) == PC.index_crc(r["index"]), i
            if i in sample:
                got = dict(index=idx, n_faces=m.n_faces, n_points=m.n_points, has_uv=True, has_nrm=True,
                           points=mem.to_host(ptr[i]["pos"], np.float32, 8 * m.n_points).reshape(-1, 8))
                PC.check_frame(r, got, "interleaved", i)
    finally:
        mem.free_all(); cd.close()


def decode_dev_counts(cd, mem, files):
    """Interleaved device outputs for every file; nothing is copied back here."""
    import uvol
    n = len(files); metas = (uvol.DecodedPoints * n)(); ptr = []
    for i, f in enumerate(files):
        nf, mv = cd.drc_info(f); metas[i].cap_faces = nf; metas[i].cap_points = mv
        row = dict(index=mem.alloc(12 * nf), pos=mem.alloc(32 * mv)); metas[i].pos = row["pos"]; metas[i].index = row["index"]; ptr.append(row)
    return cd.decode_mesh_batch_points(files, layout="interleaved", on_device=True, metas=metas), metas, None, ptr
