"""-m gpu: what makes the results of the post-process chain stale, as one table (test_gpu_despeckle.py, test_gpu_aov_shaded.py and
test_gpu_aov_lights.py each assert a part of it next to the feature they test).

  1 after a full chain (guides, accumulate, despeckle, display), pt_upload_triangles and pt_upload_materials each make the guides and
    the despeckled frame stale, make the next pt_display meter from scratch, and make the first guides afterwards drop the temporal history;
  2 the authoring calls for vertex normals, textures, bindings and uvs make shaded guides stale and leave geometric ones valid;
    pt_set_area_lights and pt_clear_area_lights do the same for lit guides (option aov_lights) and unlit ones.

The Cornell box at 16 x 12, 2 samples, option moments = 1."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, SPP = 16, 12, 2
NO_GUIDES = "%s: no guides (pt_render_aovs has not run since the scene was last uploaded)"


def fresh(api, cb_spec):
    sc = api.Scene(W, H).load(cb_spec)
    sc.set_option("moments", 1)
    sc.iterations = 4
    return sc


def einval(api, call, text=None):
    with pytest.raises(api.PtError) as e:
        call()
    assert e.value.code == api.PT_EINVAL
    if text is not None:
        assert str(e.value) == "libptamd: %s (code %d)" % (text, api.PT_EINVAL)      # (pt_last_error's text, whole)
    return str(e.value)


def bits(x):
    return np.float32(x).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------- 1: uploads
@pytest.fixture(scope="module")
def scratch_exposure(api, cb_spec):
    """what a context that has never displayed anything meters for the first frame with adapt < 1 -- and, as a control, what it
    meters when an exposure is remembered"""
    sc = fresh(api, cb_spec)
    sc.render(SPP)
    sc.display(adapt=0.25)
    scratch = sc.display_info()["exposure"]
    sc.display(metering="manual", ev=3.0)
    sc.display(adapt=0.25)
    adapted = sc.display_info()["exposure"]
    sc.close()
    assert bits(adapted) != bits(scratch)                         # (the remembered exposure does move the next one)
    return scratch


@pytest.mark.parametrize("upload", ["upload_Triangles", "upload_Materials"])
def test_upload_invalidates_the_chain(api, cb_spec, scratch_exposure, upload):
    sc = fresh(api, cb_spec)
    sc.render(SPP)
    sc.render_aovs(1, 4)
    sc.temporal_accumulate()
    sc.despeckle()
    sc.display(metering="manual", ev=3.0)                         # an exposure to remember, far from the metered one
    sc.denoise()
    sc.denoise_variance()
    sc.denoise_despeckled()
    getattr(sc, upload)()
    # the guides are stale
    einval(api, sc.denoise, NO_GUIDES % "pt_denoise")
    einval(api, sc.denoise_variance, NO_GUIDES % "pt_denoise_variance")
    einval(api, sc.denoise_despeckled, NO_GUIDES % "pt_denoise_despeckled")
    # the remembered exposure is gone: the same frame, metered from scratch
    sc.display(adapt=0.25)
    assert bits(sc.display_info()["exposure"]) == bits(scratch_exposure)
    # the first guides afterwards drop the temporal history: the next accumulate holds this frame's samples and nothing else
    sc.current_sample = 0
    sc.render(SPP)
    sc.render_aovs(1, 4)
    sc.temporal_accumulate()
    _, n = sc.read_temporal()
    assert np.all(n == float(SPP))
    # fresh guides do not bring the despeckled frame back
    sc.denoise()
    sc.denoise_variance()
    assert "has not run on the scene as uploaded" in einval(api, sc.denoise_despeckled)
    sc.despeckle()
    sc.denoise_despeckled()
    sc.close()


def test_history_survives_without_an_upload(api, cb_spec):
    """the control of the history check above: the same calls without an upload accumulate both frames"""
    sc = fresh(api, cb_spec)
    for _ in range(2):
        sc.current_sample = 0
        sc.render(SPP)
        sc.render_aovs(1, 4)
        sc.temporal_accumulate()
    _, n = sc.read_temporal()
    assert n.max() == 2.0 * SPP
    sc.close()


# ---------------------------------------------------------------------------------------------------------------- 2: authoring calls
ONE_N, ONE_UV, TEX = np.ones((1, 3, 3), np.float32), np.zeros((1, 3, 2), np.float32), np.ones((1, 1, 3), np.float32)
SHADING_CALLS = {
    "pt_set_vertex_normals": lambda sc: sc.set_vertex_normals(ONE_N),
    "pt_clear_vertex_normals": lambda sc: sc.clear_vertex_normals(),
    "pt_compute_vertex_normals": lambda sc: sc.compute_vertex_normals(30.0),
    "pt_add_texture": lambda sc: sc.add_texture(TEX),
    "pt_clear_textures": lambda sc: sc.clear_textures(),
    "pt_set_material_texture": lambda sc: sc.set_material_texture(2, 0),
    "pt_set_vertex_uvs": lambda sc: sc.set_vertex_uvs(ONE_UV),
    "pt_clear_vertex_uvs": lambda sc: sc.clear_vertex_uvs(),
}


@pytest.fixture(scope="module")
def authored(api, cb_spec):
    sc = fresh(api, cb_spec)
    sc.render(SPP)
    yield sc
    sc.close()


@pytest.mark.parametrize("name", list(SHADING_CALLS))
def test_shading_inputs_make_shaded_guides_stale(api, authored, name):
    sc = authored
    sc.add_texture(TEX)                                            # (texture 0 exists whatever ran before)
    sc.render_aovs(1, 4, shading="shaded")
    sc.denoise()
    sc.denoise_variance()
    SHADING_CALLS[name](sc)
    einval(api, sc.denoise, NO_GUIDES % "pt_denoise")
    einval(api, sc.denoise_variance, NO_GUIDES % "pt_denoise_variance")
    sc.add_texture(TEX)
    sc.render_aovs(1, 4)                                           # geometric guides read none of it
    SHADING_CALLS[name](sc)
    sc.denoise()
    sc.denoise_variance()


@pytest.mark.parametrize("name", ["pt_set_area_lights", "pt_clear_area_lights"])
def test_area_light_calls_make_lit_guides_stale(api, authored, name):
    sc = authored
    lights = [api.sphere_light((500.0, 500.0, 500.0), 100.0, radiance=(5.0, 5.0, 5.0))]
    call = (lambda: sc.set_area_lights(lights)) if name == "pt_set_area_lights" else sc.clear_area_lights
    sc.set_option("aov_lights", 1)
    sc.set_area_lights(lights)
    for shading in ("geometric", "shaded"):
        sc.render_aovs(1, 4, shading=shading)
        assert sc.stat("aov_lights") == 1                          # lit guides
        sc.denoise()
        call()
        einval(api, sc.denoise, NO_GUIDES % "pt_denoise")
        einval(api, sc.denoise_variance, NO_GUIDES % "pt_denoise_variance")
        sc.set_area_lights(lights)
    sc.set_option("aov_lights", 0)
    sc.render_aovs(1, 4)
    assert sc.stat("aov_lights") == 0                              # guides that are not lit stay valid
    call()
    sc.denoise()
    sc.denoise_variance()
    sc.clear_area_lights()
