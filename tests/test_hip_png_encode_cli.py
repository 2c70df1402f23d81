"""tools/segment.py and tools/write_slic_superpixels.py with --png-encoder gpu write the files of --png-encoder
host: the same stems, PNGs that decode to identical arrays, the same metrics."""
import importlib.util
import json
import os

import numpy as np
import pytest

from tests import png_encode_reference as ref
from tests import slic_cases as sc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool(name):
    spec = importlib.util.spec_from_file_location(name + "_tool", os.path.join(ROOT, "tools", name + ".py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def _json_line(capsys):
    return json.loads([ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")][-1])


def _pixels(path):
    from PIL import Image
    with Image.open(path) as im:
        im.load()
        return im.mode, np.asarray(im).copy()


def test_segment_writes_the_same_maps_with_either_encoder(tmp_path, capsys):
    tool = _tool("segment")
    recs = {}
    for enc in ("host", "gpu"):
        tool.main(["-o", str(tmp_path / enc), "--split", "val", "--png-encoder", enc, "--save-confidence"])
        recs[enc] = _json_line(capsys)
    host, gpu = recs["host"], recs["gpu"]
    assert gpu["png_encoder"] == "gpu" and "png_encoder" not in host
    assert set(gpu) - {"png_encoder"} == set(host) and gpu["frames"] == host["frames"] > 0
    assert set(gpu["ms_per_frame"]) == {"network", "render", "write"} and gpu["ms_per_frame"]["write"] > 0
    assert gpu["miou"] == host["miou"] and gpu["acc"] == host["acc"] and gpu["confusion"] == host["confusion"]
    for sub in ("labels", "color", "confidence"):
        names = sorted(os.listdir(tmp_path / "host" / sub))
        assert names == sorted(os.listdir(tmp_path / "gpu" / sub)) and len(names) == host["frames"]
        for n in names:
            if sub == "confidence":
                assert np.array_equal(np.load(tmp_path / "host" / sub / n), np.load(tmp_path / "gpu" / sub / n))
                continue
            mh, ah = _pixels(tmp_path / "host" / sub / n)
            mg, ag = _pixels(tmp_path / "gpu" / sub / n)
            assert mh == mg == ("L" if sub == "labels" else "RGB") and np.array_equal(ah, ag)
            # the file on disk is the encoder's format, byte for byte
            assert open(tmp_path / "gpu" / sub / n, "rb").read() == ref.encode(ag)[0]
    print("[png_encode] segment.py write ms per frame: host", host["ms_per_frame"]["write"], "gpu", gpu["ms_per_frame"]["write"], flush=True)


def test_slic_writer_writes_the_same_maps_with_either_encoder(tmp_path, capsys):
    from PIL import Image
    tool = _tool("write_slic_superpixels")
    u8 = sc.frames_u8('blobs', 40, 56, 7)                                   # [2, 3, 40, 56] uint8
    for enc in ("host", "gpu"):
        seq = tmp_path / enc / "train" / "zurich_city_00_a" / "images_aligned" / "left"
        seq.mkdir(parents=True)
        for i in range(2):
            Image.fromarray(np.ascontiguousarray(u8[i].transpose(1, 2, 0))).save(seq / f"{i:06d}.png")
        assert tool.main(["--root", str(tmp_path / enc), "--num_segments", "12", "--png-encoder", enc]) == 0
        assert "wrote 2 superpixel maps" in capsys.readouterr().out
    outs = {enc: tmp_path / enc / "train" / "zurich_city_00_a" / "sp_slic_rgb" / "left" for enc in ("host", "gpu")}
    names = sorted(os.listdir(outs["host"]))
    assert names == sorted(os.listdir(outs["gpu"])) == ["000000_slic_12.png", "000001_slic_12.png"]
    for n in names:
        mh, ah = _pixels(outs["host"] / n)
        mg, ag = _pixels(outs["gpu"] / n)
        assert mh == mg == "L" and ah.shape == (40, 56) and np.array_equal(ah, ag)
        assert open(outs["gpu"] / n, "rb").read() == ref.encode(ag)[0]
