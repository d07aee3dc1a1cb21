"""Host side of the depth output (GSRT_FLAG_DEPTH): the PFM dump and the CLI's usage errors. No device needed."""
import os
import subprocess

import numpy as np
import pytest

import gsrt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "3dgs-raytrace_amd", "bin", "gsrt_render")


@pytest.mark.parametrize("shape", [(5, 7), (5, 7, 3), (1, 1), (3, 2, 1)])
def test_dump_pfm_round_trip(tmp_path, shape):
    """Header "Pf" / "PF", "W H", scale -1.0 (little-endian), then the rows bottom to top, 4 bytes per value."""
    rng = np.random.default_rng(3)
    img = rng.normal(0.0, 10.0, shape).astype(np.float32)
    img.reshape(-1)[0] = np.float32(0.0)
    path = tmp_path / "d.pfm"
    gsrt.dump_pfm(path, img)
    raw = path.read_bytes()
    h, w = shape[:2]
    ch = 1 if len(shape) == 2 else shape[2]
    head = b"%s\n%d %d\n-1.0\n" % (b"Pf" if ch == 1 else b"PF", w, h)
    assert raw[:len(head)] == head
    body = raw[len(head):]
    assert len(body) == 4 * w * h * ch
    rows = np.frombuffer(body, "<f4").reshape(h, w, ch)
    assert rows[::-1].tobytes() == img.tobytes()  # the file's first row is the image's last
    assert raw.split(b"\n")[2] == b"-1.0"


def test_dump_pfm_rejects_other_channel_counts(tmp_path):
    for bad in (np.zeros((2, 2, 2), np.float32), np.zeros((2, 2, 4), np.float32), np.zeros(4, np.float32)):
        with pytest.raises(gsrt.GsrtError) as e:
            gsrt.dump_pfm(tmp_path / "x.pfm", bad)
        assert e.value.status == gsrt.E_ARG
    assert not (tmp_path / "x.pfm").exists()


def test_flag_value_and_abi():
    assert gsrt.FLAG_DEPTH == 0x800
    assert not gsrt.FLAG_DEPTH & (gsrt.FLAG_LUT | gsrt.FLAG_STATS | gsrt.FLAG_OUT_DUMP8 | 0xFF)
    assert gsrt.lib.gsrt_abi_version() == 2  # an addition only
    assert gsrt.lib.gsrt_depth_buffer(None) is None


@pytest.mark.parametrize("argv", [["--scene", "100", "--mode", "ref", "--depth", "d.pfm"],
                                  ["--scene", "33", "--depth", "d.pfm"],  # scene 33 defaults to REF
                                  ["--scene", "100", "--stats", "--depth", "d.pfm"],
                                  ["--scene", "100", "--depth"]])
def test_cli_depth_usage_errors(tmp_path, argv):
    """--depth with --mode ref (or a scene whose default mode is REF) or with --stats is a usage error: exit status 2
    and the usage text, decided while parsing the arguments (before any device is opened), and no file written."""
    p = subprocess.run([CLI] + argv, capture_output=True, text=True, cwd=tmp_path)
    assert p.returncode == 2, (p.returncode, p.stderr)
    assert "usage: gsrt_render" in p.stderr and "--depth" in p.stderr
    assert "gsrt_create" not in p.stderr
    assert not os.listdir(tmp_path)
