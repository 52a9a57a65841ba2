"""FG.device_geometry: <place_fiber> projects with the geometry voxelised inside the solver (fg_voxelize_into, the default)
against the same projects handed over through host arrays (device_geometry = False).  Same kernels, same inputs, same
normalisation order: everything a user sees is identical, so every comparison is exact."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HASHIN = """<settings><solver n="16"><tol>1e-6</tol><method>cg</method><mixing_rule>voigt</mixing_rule>
  <materials><matrix mu="1" lambda="3.63867684478" /><mat2 mu="3" lambda="2" /><mat1 mu="5" lambda="4" /></materials></solver>
  <actions><select_material name="mat1" /><place_fiber R="0.2" /><select_material name="mat2" /><place_fiber R="0.4" />
  %s<calc_effective_properties /></actions></settings>"""

CAPSULES = """<settings><solver n="16"><tol>1e-6</tol><method>basic</method><mixing_rule>laminate</mixing_rule>
  <materials><matrix E="1" nu="0.3" /><incl E="10" nu="0.2" /></materials></solver>
  <actions><select_material name="incl" />
  <place_fiber type="capsule" cx="0.4" cy="0.5" cz="0.45" ax="1" ay="1" az="0" L="0.5" R="0.15" />
  <place_fiber type="capsule" cx="0.6" cy="0.45" cz="0.6" ax="0" ay="1" az="1" L="0.4" R="0.12" />
  %s<calc_effective_properties /></actions></settings>"""

FULL_STAGGERED = """<settings><solver n="8"><tol>1e-6</tol><method>basic</method><gamma_scheme>full_staggered</gamma_scheme>
  <materials><matrix mu="1" lambda="1.5" /><shell mu="3" lambda="2" /><core mu="8" lambda="4" /></materials></solver>
  <actions><select_material name="shell" /><place_fiber R="0.3" cx="0.4" cy="0.5" cz="0.5" />
  <select_material name="core" /><place_fiber R="0.25" cx="0.65" cy="0.5" cz="0.5" />
  <calc_effective_properties /></actions></settings>"""


def run(xml, device, normals=None):
    from fibergen_amd import FG
    fg = FG()
    fg.device_geometry = device
    fg.set_xml(xml)
    if normals is not None:
        fg.set_normals(normals)
    assert fg.run() == 0
    return fg


def normals_or_error(fg):
    try:
        return fg.get_field("normals")
    except RuntimeError as e:
        return str(e)


@pytest.fixture(scope="module", params=["hashin", "capsules"])
def pair(request, tmp_path_factory):
    """the project run once per path, each writing its voxel table"""
    d = tmp_path_factory.mktemp(request.param)
    xml = HASHIN if request.param == "hashin" else CAPSULES
    out = [str(d / "device.txt"), str(d / "host.txt")]
    dev = run(xml % ('<write_voxel_data filename="%s" />' % out[0]), True)
    uploads = dev._lss.counter("phase_uploads")   # before anybody asks for a field
    host = run(xml % ('<write_voxel_data filename="%s" />' % out[1]), False)
    return dev, host, out, uploads


def test_results_identical(pair):
    dev, host, _out, _uploads = pair
    assert np.array_equal(np.array(dev.get_effective_property()), np.array(host.get_effective_property()))
    assert np.array(dev.get_effective_property()).shape == (6, 6)
    phi = dev.get_field("phi")
    assert np.array_equal(phi, host.get_field("phi")) and ((phi > 0) & (phi < 1)).any()
    for name in dev.get_phase_names():
        assert dev.get_volume_fraction(name) == host.get_volume_fraction(name)
        a, b = dev.get_real_volume_fraction(name), host.get_real_volume_fraction(name)
        assert a == b or (np.isnan(a) and np.isnan(b))
        assert np.array_equal(dev.get_field(name), host.get_field(name))
    assert dev.get_residuals() == host.get_residuals()
    nrm = [normals_or_error(fg) for fg in (dev, host)]
    if dev._mixing == "laminate":
        assert np.array_equal(nrm[0], nrm[1]) and np.abs(nrm[0]).max() > 0
    else:   # no normals in this project: both paths say so in the same words
        assert isinstance(nrm[0], str) and nrm[0] == nrm[1]


def test_no_host_upload_on_the_device_path(pair):
    dev, host, _out, uploads = pair
    assert uploads == 0
    assert host._lss.counter("phase_uploads") >= len(host.get_phase_names())


def test_voxel_tables_byte_identical(pair):
    dev, _host, out, _uploads = pair
    a, b = open(out[0], "rb").read(), open(out[1], "rb").read()
    assert a == b and len(a) > 16 ** 3
    head = a.split(b"\n", 1)[0].split(b"\t")
    assert (b"n_x" in head) == (dev._mixing == "laminate")   # the lazily fetched normals reach the writer


def test_full_staggered_project():
    dev, host = run(FULL_STAGGERED, True), run(FULL_STAGGERED, False)
    assert dev._lss.counter("phase_uploads") == 0 and host._lss.counter("phase_uploads") == 3
    assert np.array_equal(np.array(dev.get_effective_property()), np.array(host.get_effective_property()))
    assert np.array_equal(dev.get_field("phi"), host.get_field("phi"))
    for name in dev.get_phase_names():
        assert dev.get_volume_fraction(name) == host.get_volume_fraction(name)
        assert dev.get_real_volume_fraction(name) == host.get_real_volume_fraction(name)


VOIGT_CAPSULES = CAPSULES.replace("<mixing_rule>laminate", "<mixing_rule>voigt")


def test_injected_normals():
    """FG.set_normals on both paths alike.  Where the voxeliser makes no normals (Voigt mixing, no normals="1") the injected
    array is what the solver holds, and the device path uploads that one array and nothing else.  Where it does (laminate
    mixing), the voxeliser's normals replace the injected ones on the host path, and the device path does the same."""
    rng = np.random.default_rng(5)
    n = rng.standard_normal((3, 16, 16, 16))
    n /= np.sqrt((n * n).sum(axis=0))
    dev, host = run(VOIGT_CAPSULES % "", True, normals=n), run(VOIGT_CAPSULES % "", False, normals=n)
    assert np.array_equal(dev.get_field("normals"), n) and np.array_equal(host.get_field("normals"), n)
    assert dev._lss.counter("phase_uploads") == 1
    assert np.array_equal(np.array(dev.get_effective_property()), np.array(host.get_effective_property()))
    dev, host, plain = run(CAPSULES % "", True, normals=n), run(CAPSULES % "", False, normals=n), run(CAPSULES % "", False)
    assert np.array_equal(dev.get_field("normals"), host.get_field("normals"))
    assert np.array_equal(host.get_field("normals"), plain.get_field("normals"))
    assert np.array_equal(np.array(dev.get_effective_property()), np.array(host.get_effective_property()))
    assert dev._lss.counter("phase_uploads") == 0


def test_second_geometry_in_one_fg():
    """init_phase again on a live FG (a phase field injected after the first run): the marks of the device path do not
    outlive their geometry, and both paths still agree"""
    x = (np.arange(16) + 0.5) / 16 - 0.5
    ball = ((x[:, None, None] ** 2 + x[None, :, None] ** 2 + x[None, None, :] ** 2) < 0.09).astype(float)
    out = []
    for device in (True, False):
        fg = run(CAPSULES % "", device)
        fg.set_phase_field("incl", ball)
        fg.init_phase()
        assert not fg._phi_on_device and not fg._normals_on_device
        out.append((fg.get_field("phi"), fg.get_field("normals")))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    assert np.array_equal(out[0][0][1], ball)
