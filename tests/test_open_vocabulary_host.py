"""Host side of K36 (no GPU): the new C entries in the header, the binding and the library with the ABI untouched, their refusals
(they return before the first HIP call), the Segmenter's vocabulary refusals with the model construction patched out, the parsing of
tools/segment.py --classes and the palette's determinism."""
import ctypes
import importlib.util
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "tests", "configs", "finetune_dsec_synthetic.yaml")


def test_entries_are_declared_bound_and_exported():
    from openess_amd import _lib
    header = open(os.path.join(ROOT, "include", "oess.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, count in (("oess_segment_render_grouped", 21), ("oess_head_render", 21)):
        m = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)", code)
        assert m and len(m.group(1).split(',')) == count
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == count and args[2] is ctypes.c_longlong
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    lib = _lib.load()
    assert lib.oess_abi_version() == 13 == _lib.ABI_VERSION and int(re.search(r"#define\s+OESS_ABI_VERSION\s+(\d+)", header).group(1)) == 13
    assert [lib.oess_head_render_max_names(C) for C in (0, 1, 32, 64, 65)] == [0, 6144, 372, 189, 0]


def test_entries_refuse_on_the_host():
    """every refusal returns before the first HIP call: the pointers are never read"""
    from openess_amd import _lib
    lib = _lib.load()
    ok = dict(x=4096, ps=36, B=2, K=11, P=36, h=3, w=4, H=6, W=8, offs=28672, palette=8192, alpha256=128, min_conf=0.0, ignore=255,
              labels=16384)

    def grouped(**kw):
        a = dict(ok, **kw)
        return lib.oess_segment_render_grouped(a['x'], 0, a['ps'], a['B'], a['K'], a['P'], a['h'], a['w'], a['H'], a['W'], 0, a['offs'],
                                               a['palette'], None, a['alpha256'], a['min_conf'], a['ignore'], a['labels'], None, 24576, None)

    def head(**kw):
        a = dict(dict(ok, ps=32, C=32, weight=32768), **kw)
        return lib.oess_head_render(a['x'], 1, a['ps'], a['B'], a['C'], a['H'], a['W'], a['weight'], None, a['K'], a['P'], a['offs'],
                                    a['palette'], None, a['alpha256'], a['min_conf'], a['ignore'], a['labels'], None, 24576, None)
    shared = (dict(x=None), dict(palette=None), dict(K=0), dict(K=256, P=300, ps=300), dict(P=10), dict(P=1025, ps=1025),
              dict(ignore=10), dict(ignore=256), dict(alpha256=-1), dict(alpha256=257), dict(min_conf=float('nan')), dict(min_conf=-1e-3),
              dict(B=0), dict(H=0), dict(W=-2), dict(ps=1 << 62))
    for bad in shared + (dict(offs=None), dict(ps=35), dict(h=0), dict(w=-1), dict(B=1 << 16, H=1 << 16), dict(B=1 << 16, h=1 << 16)):
        assert grouped(**bad) == -22, bad
    for bad in shared + (dict(weight=None), dict(offs=None), dict(ps=31), dict(C=0), dict(C=65, ps=65), dict(P=373, K=11),
                         dict(C=64, ps=64, P=190)):
        assert head(**bad) == -22, bad


def test_wrappers_refuse_a_cpu_tensor():
    from openess_amd import hip
    with pytest.raises(ValueError, match="no CPU fallback"):
        hip.segment_render(torch.zeros(1, 3, 2, 2), class_offsets=[0, 1, 3])
    with pytest.raises(ValueError, match="no CPU fallback"):
        hip.vocab_render(torch.zeros(1, 3, 2, 2), torch.zeros(2, 3))


def _bare_segmenter(is_event=True, probe=False, ignore=255):
    """a Segmenter without its networks: what the vocabulary refusals look at"""
    from openess_amd.inference import Segmenter
    seg = Segmenter.__new__(Segmenter)
    model = SimpleNamespace(if_linear_probing=probe)
    seg.trainer = SimpleNamespace(models_dict={'back_end': model, 'model_recon': model})
    seg.settings = SimpleNamespace(clip_text_checkpoint=None, clip_bpe_path=None)
    seg.is_event, seg.precision, seg.device, seg.ignore_label = is_event, 'bf16', torch.device('cpu'), ignore
    seg.num_classes, seg.palette = 11, torch.zeros(11, 3, dtype=torch.uint8)
    seg._own, seg._vocab = (seg.num_classes, seg.palette), None
    return seg


def _unit(P, D=512):
    t = torch.randn(P, D, generator=torch.Generator().manual_seed(P))
    return t / t.norm(dim=1, keepdim=True)


@pytest.mark.parametrize("is_event", [True, False], ids=["event", "frame2recon"])
def test_vocabulary_refusals_before_any_launch(is_event, tmp_path):
    seg = _bare_segmenter(is_event)
    cases = [(dict(T=_unit(3, 256)), "width 512"),
             (dict(T=_unit(3)[0]), "float \\[P, 512\\]"),
             (dict(T=torch.zeros(3, 512, dtype=torch.int64)), "float \\[P, 512\\]"),
             (dict(T=_unit(256)), "at most 255 classes"),
             (dict(T=_unit(1025), class_offsets=[0, 1025]), "at most 1024 names"),
             (dict(T=_unit(7), class_offsets=[0, 2, 2, 7]), "class_offsets must start at 0"),
             (dict(T=_unit(7), class_offsets=[1, 2, 7]), "class_offsets must start at 0"),
             (dict(T=_unit(7), class_offsets=[0, 2, 6]), "class_offsets must start at 0"),
             (dict(T=_unit(7), class_offsets=[0, 2, 3, 7], names=["a", "b"]), "one entry per class"),
             (dict(T=_unit(7), class_offsets=[0, 2, 3, 7], palette=np.zeros((7, 3), np.uint8)), "palette must be uint8 \\[3, 3\\]"),
             (dict(T=_unit(7), class_offsets=[0, 2, 3, 7], palette=np.zeros((3, 3), np.int32)), "palette must be uint8")]
    for kw, message in cases:
        with pytest.raises(ValueError, match=message):
            seg.set_vocabulary_embeddings(**kw)
        assert seg._vocab is None and seg.num_classes == 11
    with pytest.raises(ValueError, match="would be a class"):
        _bare_segmenter(is_event, ignore=2).set_vocabulary_embeddings(_unit(7), [0, 2, 3, 7])
    probe = _bare_segmenter(is_event, probe=True)
    with pytest.raises(ValueError, match="linear-probe"):
        probe.set_vocabulary_embeddings(_unit(3))
    with pytest.raises(ValueError, match="linear-probe"):
        probe.set_vocabulary(["road", "car"])
    # set_vocabulary: the CLIP files
    with pytest.raises(ValueError, match="clip_text_checkpoint"):
        seg.set_vocabulary(["road", "car"])
    with pytest.raises(ValueError, match="clip_text_checkpoint"):
        seg.set_vocabulary(["road", "car"], clip_bpe_path=str(tmp_path / "merges.txt"))
    with pytest.raises(ValueError, match="file not found"):
        seg.set_vocabulary(["road", "car"], clip_text_checkpoint=str(tmp_path / "absent.pt"), clip_bpe_path=str(tmp_path / "absent.txt"))
    with pytest.raises(ValueError, match="merge must be"):
        seg.set_vocabulary(["road", "car"], merge='sum')
    seg.reset_vocabulary()
    assert seg.num_classes == 11 and seg._vocab is None


def test_a_vocabulary_on_frame2recon_needs_no_device_until_it_predicts():
    """frame2recon keeps the matrix, the offsets, the names and the palette; nothing is launched by set_vocabulary_embeddings"""
    from openess_amd.inference import voc_palette
    seg = _bare_segmenter(is_event=False)
    seg.set_vocabulary_embeddings(_unit(7).double(), [0, 2, 3, 7], names=["road", ["car", "cab"], "person"][:3])
    v = seg._vocab
    assert (v.K, v.P, v.offsets, v.grouped) == (3, 7, [0, 2, 3, 7], True) and v.T.dtype == torch.float32
    assert seg.num_classes == 3 and np.array_equal(seg.palette.numpy(), voc_palette(3))
    assert seg.vocabulary == [{'id': 0, 'names': ['road'], 'color': [0, 0, 0]}, {'id': 1, 'names': ['car', 'cab'], 'color': [128, 0, 0]},
                              {'id': 2, 'names': ['person'], 'color': [0, 128, 0]}]
    seg.set_vocabulary_embeddings(_unit(4))
    assert (seg._vocab.K, seg._vocab.grouped, seg._vocab.names) == (4, False, None) and seg.vocabulary[3]['names'] is None
    seg.reset_vocabulary()
    assert seg.num_classes == 11 and seg.palette.shape == (11, 3)


def test_palette_is_deterministic():
    from openess_amd.inference import voc_palette
    a, b = voc_palette(40), voc_palette(40)
    assert np.array_equal(a, b) and a.dtype == np.uint8 and not a[0].any() and np.array_equal(voc_palette(7), a[:7])
    assert len({tuple(c) for c in a.tolist()}) == 40


def _tool():
    spec = importlib.util.spec_from_file_location("segment_tool", os.path.join(ROOT, "tools", "segment.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_cli_parses_classes_as_a_list_and_as_a_file(tmp_path, capsys):
    tool = _tool()
    out = str(tmp_path / "out")
    ckpt, bpe = tmp_path / "clip.pt", tmp_path / "merges.txt"
    ckpt.write_bytes(b"x"), bpe.write_text("x")
    files = ["--clip-text-checkpoint", str(ckpt), "--bpe", str(bpe)]

    def parse(argv):
        ap = tool.build_parser()
        a = ap.parse_args(["-o", out] + argv)
        tool.check_args(ap, a)
        return a.vocabulary
    v = parse(["--classes", "road, car|vehicle ,person"] + files)
    assert v == dict(classes=["road", ["car", "vehicle"], "person"], merge="max", templates="single", clip_text_checkpoint=str(ckpt),
                     clip_bpe_path=str(bpe))
    (tmp_path / "classes.txt").write_text("road\n\ncar|vehicle\nperson\n")
    (tmp_path / "templates.txt").write_text("a photo of a {}.\n")
    v = parse(["--classes", str(tmp_path / "classes.txt"), "--merge", "mean", "--templates", str(tmp_path / "templates.txt")] + files)
    assert v['classes'] == ["road", ["car", "vehicle"], "person"] and v['merge'] == "mean" and v['templates'] == str(tmp_path / "templates.txt")
    assert parse([]) is None
    cases = {
        "merge_alone": (["--merge", "mean"], "--merge needs --classes"),
        "bpe_alone": (["--bpe", str(bpe)], "--bpe needs --classes"),
        "no_clip_files": (["--classes", "road,car"], "--clip-text-checkpoint and --bpe"),
        "missing_checkpoint": (["--classes", "road,car", "--clip-text-checkpoint", str(tmp_path / "absent.pt"), "--bpe", str(bpe)], "not found"),
        "missing_templates": (["--classes", "road,car", "--templates", str(tmp_path / "absent.txt")] + files, "not found"),
        "empty_class": (["--classes", "road,|,car"] + files, "empty class"),
        "no_class": (["--classes", " , "] + files, "no class"),
        "too_many": (["--classes", ",".join(f"c{i}" for i in range(256))] + files, "at most 255 classes"),
        "probe": (["--classes", "road,car", "--settings", "PROBE"] + files, "linear-probe"),
    }
    import yaml
    cfg = yaml.load(open(CFG), yaml.Loader)
    probe_yaml = tmp_path / "probe.yaml"
    cfg['clip'].update(if_linear_probing=True, if_finetuning=False)
    probe_yaml.write_text(yaml.dump(cfg))
    for name, (argv, message) in cases.items():
        with pytest.raises(SystemExit) as e:
            tool.main(["-o", out] + [str(probe_yaml) if t == "PROBE" else t for t in argv])
        assert e.value.code == 2, name
        assert message in capsys.readouterr().err, name
    assert not os.path.exists(out)                                        # refused before anything is written
