"""A frame left in flight: what a scene handle does when something else is asked of it between render_launch and
render_finish.  One frame is in flight per scene at a time (its counters and item sums are the scene's), so a second launch,
a change of settings, a film's pass and the end of the handle each wait for the frame first -- and the frame's buffer, a torch
tensor on the launch's stream, holds the frame afterwards, bit for bit what the synchronous render of the same handle gives.
Both routes: the streaming route on a small mesh, the local-pool route on seven spheres."""
import numpy as np
import pytest
import torch

import rayrs_amd
from rayrs_amd import _ffi, procedural, scenes
from test_gpu_render import assert_same_frame

pytestmark = pytest.mark.gpu

HDRI = procedural.make_hdri(64, 32)
INVALID_ARG = -1   # include/rayrs_hip.h RAYRS_INVALID_ARG
ROUTES = {"streaming": (lambda: scenes.mesh_scene(3), 64, 48, 4), "local_pool": (scenes.cook_torrance_spheres_metallic, 48, 32, 2)}
SEEDS = (11, 12)


class Flight:
    """A scene handle of a route, the synchronous frames of SEEDS on it, and launches into fresh buffers on a side stream."""

    def __init__(self, route):
        fn, w, h, self.spp = ROUTES[route]
        cam_args, objs, self.heur = fn()
        self.objs = objs
        self.cam = rayrs_amd.Camera(*scenes.camera_for_resolution(cam_args, w, h))
        self.scene = self.new_scene()
        assert self.scene.info()["local_pool"] == (1 if route == "local_pool" else 0)
        self.ref = {seed: rayrs_amd.render(self.scene, self.cam, self.spp, seed=seed, out_f64=True)[0] for seed in SEEDS}
        assert not np.array_equal(self.ref[SEEDS[0]], self.ref[SEEDS[1]])
        self.stream = torch.cuda.Stream()

    def new_scene(self):
        return rayrs_amd.Scene(self.objs, 1e-6, 1e6, self.heur, HDRI, device=0)

    def launch(self, scene, seed):
        with torch.cuda.stream(self.stream):
            buf = torch.zeros((self.cam.y_pixels(), self.cam.x_pixels(), 3), dtype=torch.float64, device="cuda")
            rayrs_amd.render_launch(scene, self.cam, rayrs_amd.make_params(self.spp, seed=seed, out_f64=True), buf.data_ptr(),
                                    torch.cuda.current_stream().cuda_stream)
        return buf

    def holds(self, buf, seed):
        assert_same_frame(buf.cpu().numpy(), self.ref[seed])


@pytest.fixture(scope="module", params=list(ROUTES))
def flight(request):
    return Flight(request.param)


def test_a_second_launch_waits_for_the_first(flight):
    a = flight.launch(flight.scene, SEEDS[0])
    b = flight.launch(flight.scene, SEEDS[1])
    st = rayrs_amd.render_finish(flight.scene)
    assert st["paths"] == flight.cam.x_pixels() * flight.cam.y_pixels() * flight.spp
    flight.holds(a, SEEDS[0])
    flight.holds(b, SEEDS[1])


@pytest.mark.parametrize("how", ["set_tuning", "lab_set"])
def test_new_settings_wait_for_the_frame(flight, how):
    buf = flight.launch(flight.scene, SEEDS[0])
    getattr(flight.scene, how)()   # (the defaults again: the next test's frames are these frames)
    flight.stream.synchronize()
    flight.holds(buf, SEEDS[0])
    with pytest.raises(_ffi.RayrsError) as e:   # nothing is pending any more
        rayrs_amd.render_finish(flight.scene)
    assert e.value.status == INVALID_ARG


def test_a_film_on_a_busy_scene(flight):
    buf = flight.launch(flight.scene, SEEDS[0])
    film = rayrs_amd.Film(flight.scene, flight.cam, sample_chunk=4, seed=SEEDS[1])
    film.render(4)
    flight.stream.synchronize()
    flight.holds(buf, SEEDS[0])
    fresh = rayrs_amd.Film(flight.scene, flight.cam, sample_chunk=4, seed=SEEDS[1])
    fresh.render(4)
    assert_same_frame(film.image(out_f64=True), fresh.image(out_f64=True))
    film.close()
    fresh.close()


def test_closing_the_scene_waits_for_the_frame(flight):
    scene = flight.new_scene()
    buf = flight.launch(scene, SEEDS[1])
    scene.close()
    torch.cuda.synchronize()
    flight.holds(buf, SEEDS[1])
