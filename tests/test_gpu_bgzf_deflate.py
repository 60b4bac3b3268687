"""The BGZF encoder on the GPU (secedo_amd.bgzf_deflate, bgzf_deflate_kernels.hip): the inputs and checks of
tests/test_bgzf_deflate_cpu.py, and byte for byte the output of the host program built from the same header, which is
what catches a race between lanes. Our own decoder (secedo_amd.bgzf_inflate) reads every file back."""
import numpy as np
import pytest

import secedo_amd
from secedo_amd import variant
from tests import bgzf_deflate_cases as dc

pytestmark = pytest.mark.gpu

CASES = dc.cases()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("deflate_host")
    return {name: dc.host_encode(data, tmp, name) for name, data in CASES.items()}


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_equals_host_and_zlib_reads_it(host, tmp_path, name):
    data = CASES[name]
    raw = secedo_amd.bgzf_deflate(data)
    dc.check_file(raw, data)
    assert raw == host[name]
    assert secedo_amd.bgzf_deflate(data) == raw  # two runs give the same bytes
    path = tmp_path / "x.gz"
    path.write_bytes(raw)
    assert secedo_amd.bgzf_inflate(str(path)).tobytes() == data  # our own decoder accepts our own encoder


def test_stats_of_a_call():
    data = CASES["sam_%d" % (2 * dc.CUT + 1)] + CASES["random_65280"]
    raw = secedo_amd.bgzf_deflate(data)
    st = variant.vcf_stats()
    assert st["output"] == "bgzf" and st["files"] == 1 and st["text_bytes"] == len(data)
    assert st["compressed_bytes"] == len(raw) and st["blocks"] == 4 and st["stored_blocks"] == 1


def test_one_launch_with_300_tiny_inputs(host, tmp_path):
    rng = np.random.default_rng(23)
    sam = dc.gw.sam_like_text(40)
    inputs = []
    for k in range(300):
        n = 0 if k % 7 == 0 else int(rng.integers(1, 400))
        o = int(rng.integers(0, len(sam) - 400))
        inputs.append(sam[o:o + n])
    inputs[5] = CASES["sam_%d" % (dc.CUT + 1)]  # one input of two members among them
    files = variant.bgzf_deflate_many(inputs)
    st = variant.vcf_stats()
    assert len(files) == 300 and st["files"] == 300
    assert st["blocks"] == sum(-(-len(d) // dc.CUT) for d in inputs) and st["compressed_bytes"] == sum(map(len, files))
    for k, (raw, data) in enumerate(zip(files, inputs)):
        dc.check_file(raw, data, with_tokens=k < 20)
        if not data:
            assert raw == dc.gw.EOF_MEMBER
    assert files[5] == host["sam_%d" % (dc.CUT + 1)]
    for k in (1, 2, 3, 150, 299):  # the batch gives what a launch of its own gives
        assert files[k] == secedo_amd.bgzf_deflate(inputs[k]), k
    assert files[1] == dc.host_encode(inputs[1], tmp_path, "tiny")


@pytest.mark.parametrize("which", ["vcf", "sam"])
def test_ratio_against_zlib_level_1(which):
    """Compressed size over zlib's at level 1 on the same blocks (the bound and the measured quotient are in
    tests/bgzf_deflate_cases.py); no block of compressible text is stored; no member exceeds 64 KiB."""
    data = dc.vcf_like_text() if which == "vcf" else dc.gw.sam_like_text(4000)
    bound = dc.RATIO_VCF_BOUND if which == "vcf" else dc.RATIO_SAM_BOUND
    raw = secedo_amd.bgzf_deflate(data)
    members = dc.check_file(raw, data, with_tokens=False)
    assert variant.vcf_stats()["stored_blocks"] == 0
    assert all(((m[1][0] >> 1) & 3) == 1 for m in members)  # BTYPE 1 everywhere
    ours, (z1, z6) = dc.payload_bytes(raw), dc.zlib_sizes(data)
    print("%s: %d bytes of text, ours %d, zlib level 1 %d, level 6 %d, ours / level 1 = %.4f"
          % (which, len(data), ours, z1, z6, ours / z1))
    assert ours <= bound * z1
