"""What tests/test_upscale.py and tests/test_upscale_wide.py share in driving a Renderer through guided upscaling: the cache of the CPU
side of the model, the colour a source holds as the handle reads it back, the check of one call against a numpy model, and the
snapshots of what a call must leave alone.  `rt` is the package, handed in by the caller; nothing here imports it."""
import numpy as np

from tests.edge_resolve_model import coverage_np, scene_of
from tests.preview_model import same_bits
from tests.upscale_model import DENOISED, HISTORY, LINEAR, colour_of, output_hits


class Cpu:
    """The CPU side of the model, computed once per camera and shared: cpu.hits(prec, scene_id, cam, F) the output pixels' hits (F = 1: the
    traced pixels' first-hit guides), cpu.layers(prec, scene_id, cam, G) the coverage layers.  Nothing here is changed by a test."""
    def __init__(self, rt, oracle):
        self.rt, self.oracle, self.cache = rt, oracle, {}

    def _get(self, key, make):
        if key not in self.cache:
            self.cache[key] = make()
        return self.cache[key]

    @staticmethod
    def _name(scene_id):
        """What a scene is cached under: its id, or the "name" of scene tables handed in as they are (tests/range_scene.py)."""
        return scene_id["name"] if isinstance(scene_id, dict) else scene_id

    def hits(self, prec, scene_id, cam, F):
        rows = np.arange(cam.img_height)
        return self._get(("hits", prec, self._name(scene_id), bytes(cam), F),
                         lambda: output_hits(self.oracle, prec, scene_of(self.rt, scene_id, prec), cam, rows, F))

    def layers(self, prec, scene_id, cam, G):
        rows = np.arange(cam.img_height)
        return self._get(("layers", prec, self._name(scene_id), bytes(cam), G),
                         lambda: coverage_np(self.oracle, prec, scene_of(self.rt, scene_id, prec), cam, rows, G)[:2])


def colour(r, source, adaptive=False):
    """colour_of's (c, has) of a source, read back from the handle."""
    if source == DENOISED:
        return colour_of(DENOISED, g=r.read_denoised())
    if source == LINEAR:
        lin = r.read_linear()
        n = r.adaptive_state()[0] if adaptive else np.full(lin.shape[:2], r.accumulated_samples, np.int32)
        return colour_of(LINEAR, linear=lin, n=n)
    C, M = r.history()
    return colour_of(HISTORY, C=C, M=M)


def _model(np_model, r, cpu, prec, scene_id, cam, source, setting, G, adaptive):
    F, sn, sa, sz, flag = setting
    c, has = colour(r, source, adaptive)
    _, N, A, Z = cpu.hits(prec, scene_id, cam, 1)
    ids, counts = cpu.layers(prec, scene_id, cam, G)
    return (c,) + tuple(np_model(c, has, N, A, Z, ids, counts, G * G, cpu.hits(prec, scene_id, cam, F), F, sn, sa, sz, flag))


def model(np_model, r, cpu, prec, scene_id, cam, source, setting, G, adaptive=False):
    """np_model's (image, covered) of `setting` on what the handle holds."""
    return _model(np_model, r, cpu, prec, scene_id, cam, source, setting, G, adaptive)[1:]


def check(upscale, np_model, r, cpu, prec, scene_id, cam, source, setting, G, where, adaptive=False):
    """upscale -- r.upscale or r.upscale_wide -- at `setting` with the layers of lattice G against np_model, every pixel, and the count;
    returns the image."""
    F, sn, sa, sz, flag = setting
    where = where + (source, setting, G)
    c, want, covered = _model(np_model, r, cpu, prec, scene_id, cam, source, setting, G, adaptive)
    count = upscale(F, source, sn, sa, sz, flag)
    out = r.read_upscaled()
    H, W = c.shape[:2]
    assert out.shape == want.shape == (F * H, F * W, 3) and out.dtype == want.dtype == c.dtype, where
    assert same_bits(out, want), (where, int((out != want).any(axis=-1).sum()))
    assert count == int(covered.sum()), (where, count, int(covered.sum()))
    ptr, nbytes = r.upscaled_device_ptr()
    assert ptr and nbytes == out.nbytes, where
    return out


def check_guides(r, cpu, prec, scene_id, cam, where):
    """The traced pixels' guides of the model are the handle's, bit for bit."""
    _, N, A, Z = cpu.hits(prec, scene_id, cam, 1)
    for name, a, b in zip(("normal", "albedo", "depth"), r.guides(), (N, A, Z)):
        assert same_bits(a, b), (where, name)


def _bits(r):
    """What a refused call must leave alone."""
    return {"upscaled": r.read_upscaled(), "denoised": r.read_denoised(), "fb": r.read_framebuffer(), "linear": r.read_linear(),
            "samples": np.array([r.accumulated_samples])}


def _everything(r):
    out = {"fb": r.read_framebuffer(), "linear": r.read_linear(), "denoised": r.read_denoised(), "temporal": r.history()[0], "length": r.history()[1],
           "base": r.history_base()[0], "base_length": r.history_base()[1], "plan": r.history_plan_lengths()}
    out["counts"], out["err"] = r.adaptive_state()
    out["normal"], out["albedo"], out["depth"] = r.guides()
    out["ids"], out["layer_counts"], out["layer_normal"], out["layer_depth"] = r.coverage()
    return out
