"""The (scene, parameters) cases of tests/test_adaptive_rule.py, with their oracle samples and reference results, shared with
tests/test_adaptive_reference.py, which checks on the CPU that the reference decides every pixel of every case."""
import collections

import adaptive_reference as ar
from conftest import load_scene, random_scene

from pathtracer_cuda_interactive_amd import PT_BVH_SORT_REFERENCE, PT_RENDER_NEE, PT_TRAVERSAL_PRUNED

W, H = 40, 30
SCENES = ["scene1", "cbox", "random3", "random3_black"]

# spp, batch_spp, max_spp, max_error, min_luminance, p_value
Rule = collections.namedtuple("Rule", "spp batch max_spp max_error min_luminance p_value")
RULES = [Rule(4, 4, 32, 0.2, 0.01, 0.0), Rule(1, 3, 32, 0.2, 0.0, 0.05), Rule(2, 5, 31, 0.3, 0.0, 0.3),
         Rule(4, 4, 32, 0.1, 0.5, 0.001), Rule(3, 3, 32, 0.05, 0.01, 0.9), Rule(4, 7, 30, 0.02, 0.0, 0.5)]
P_VALUES = sorted({r.p_value for r in RULES})

# A frame: what pt_render_params holds beyond the camera.  stride 0 = the default (max_spp); rows = (begin, end, stride) or None.
Frame = collections.namedtuple("Frame", "scene w h flags traversal stride rows", defaults=(W, H, 0, 0, 0, None))

# name -> (frame, rule): the extra cases of the every-pixel test
VARIANTS = {
    "nee": (Frame("cbox", flags=PT_RENDER_NEE), RULES[3]),
    # the oracle never prunes, and pruned traversal is not guaranteed bit-exact: the GPU test takes this case's
    # samples from pruned pt_render calls at spp = 1; the oracle's samples stand in for them in the CPU check of the case
    "pruned": (Frame("random3", traversal=PT_TRAVERSAL_PRUNED), RULES[0]),
    "defaults": (Frame("scene1"), Rule(1, 0, 0, 0.2, 0.01, 0.0)),
    "stride": (Frame("random3", stride=64), RULES[0]),
    "rows": (Frame("scene1", rows=(1, 29, 3)), RULES[2]),
}

# The list-size cases: exactly k pixels continue after round 0.  One rule, max_error chosen per k from the reference.
LIST_RULE = Rule(4, 4, 12, None, 0.01, 0.0)
LIST_FRAME = Frame("random3", 48, 36)             # at 40 x 30 the ranks 63 and 64 tie
LIST_SIZES = [0, 1, 63, 64, 65, 255, 256, 257]
SMALL_FRAMES = {"1x1": (Frame("random3", 1, 1), Rule(2, 3, 16, 0.05, 0.01, 0.0)),
                "65x1": (Frame("random3", 65, 1), Rule(2, 3, 16, 0.1, 0.01, 0.0))}

# The edges of the rule: every pixel stops at once; none but the constant ones ever does.
ALL_STOP = (Frame("scene1"), Rule(4, 4, 32, 1e6, 0.01, 0.0))
NONE_STOP = (Frame("random3"), Rule(4, 4, 16, 1e-12, 0.01, 0.0))
BLACK = [(Frame("random3_black"), RULES[1]), (Frame("random3_black"), Rule(4, 4, 16, 0.2, 0.0, 0.0))]

# Passes under an explicit scratch budget, and the call forms
PASSES = (Frame("random3"), RULES[0])
FORMS = (Frame("cbox"), RULES[0])

# One handle, many calls: the buffers grow and are reused
SEQUENCE = [(Frame("scene1"), RULES[0]), (Frame("scene1", 8, 4), RULES[0]), (Frame("scene1", 64, 48), Rule(4, 4, 16, 0.2, 0.01, 0.0)),
            (Frame("scene1"), RULES[2])]
OVERLAP = (Frame("scene1"), RULES[5])


def every_case():
    """name -> (frame, rule) of every case a GPU test runs, the list-size cases aside (their max_error comes from list_case)."""
    out = {f"{s}-{i}": (Frame(s), r) for s in SCENES for i, r in enumerate(RULES)}
    out.update(VARIANTS)
    out.update(SMALL_FRAMES)
    out.update({"all_stop": ALL_STOP, "none_stop": NONE_STOP, "black-4": BLACK[1], "sequence-8x4": SEQUENCE[1],
                "sequence-64x48": SEQUENCE[2]})
    return out


_scenes, _samples = {}, {}


def scene(name):
    """(HostScene, desc), cached."""
    if name not in _scenes:
        if name.startswith("random"):
            hs = random_scene(3)
            if name.endswith("_black"):
                hs.set_background((0, 0, 0))
            _scenes[name] = (hs, hs.finalize(PT_BVH_SORT_REFERENCE))
        else:
            _scenes[name] = load_scene(name)
    return _scenes[name]


def params(frame, spp):
    """pt_render_params of a frame for a call whose first round has spp samples."""
    hs, _ = scene(frame.scene)
    p = hs.render_params(frame.w, frame.h, spp)
    p.flags, p.traversal, p.stream_stride = frame.flags, frame.traversal, frame.stride
    if frame.rows:
        p.row_begin, p.row_end, p.row_stride = frame.rows
    return p


def frame_samples(oracle, frame, max_spp):
    """The oracle's samples of a frame, computed once per (frame, stride) and never changed: [rows * W, >= max_spp, 3]."""
    stride = frame.stride or max_spp
    key = (frame._replace(traversal=0), stride)              # the oracle has one traversal
    if key not in _samples or _samples[key].shape[1] < max_spp:
        s = ar.samples(oracle, scene(frame.scene)[1], params(frame, 1), max_spp, stride)
        s.setflags(write=False)
        _samples[key] = s
    return _samples[key][:, :max_spp]


def reference(oracle, frame, rule, scratch_bytes=None):
    """(pt_render_params, adaptive_reference.Expected) of a case."""
    _, max_spp = ar.defaults(rule.spp, rule.batch, rule.max_spp)
    s = frame_samples(oracle, frame, max_spp)
    return params(frame, rule.spp), ar.expected(s, *rule, scratch_bytes=scratch_bytes)


def list_case(oracle, k):
    """The rule under which exactly k pixels of LIST_FRAME continue after round 0 (None where the ranks tie)."""
    s = frame_samples(oracle, LIST_FRAME, LIST_RULE.max_spp)
    probe = LIST_RULE._replace(max_error=1.0, max_spp=LIST_RULE.spp)            # one checkpoint: err at n = spp
    _, err0, _ = ar.rule(s, probe.spp, probe.batch, probe.max_spp, probe.max_error, probe.min_luminance, ar.quantile(probe.p_value))
    t = ar.threshold_for(err0, k)
    return None if t is None else LIST_RULE._replace(max_error=float(t))
