"""The host-side GPU layout code (optix-renderer_amd/host/gpu_layout.cpp) checked on the CPU: tests/c/gpu_layout_check
loads a scene, builds the reference-layout BVH and checks the flattened tree, the wide collapse, the top-first
numbering, the isolated-sphere marks, nee_finite and the corrupt-BVH errors against properties it derives on its own;
`tables` checks the block spiral and the lens-stream tables. One run per scene, the smallest that reach each branch."""
import os
import re
import subprocess

import pytest

import scenegen

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(REPO, "tests", "c", "bin", "gpu_layout_check")

DIELECTRIC_SPHERE = '<point name="center" value="0.445800 0.332100 0.376700" />'
MIRROR_SPHERE = '<point name="center" value="-0.421400 0.332100 -0.280000" />'
DIFFUSE = '<bsdf type="diffuse"><color name="albedo" value="0.5 0.5 0.5"/></bsdf>'


def run(*args):
    r = subprocess.run([CHECK, *args], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


@pytest.fixture(scope="module")
def cbox(tmp_path_factory):
    """(path, text) of the Cornell box c1: three meshes, a mirror and a dielectric sphere, the light mesh"""
    path = scenegen.cbox_xml(str(tmp_path_factory.mktemp("layout")), "c1", width=64, height=64, spp=1)
    return path, open(path).read()


def variant(cbox, name, edit):
    path, text = cbox
    new = edit(text)
    assert new != text
    out = os.path.join(os.path.dirname(path), name + ".xml")
    with open(out, "w") as f:
        f.write(new)
    return out


def only_shapes(cbox, name, shapes):
    """The Cornell box's camera and integrator around `shapes` alone"""
    return variant(cbox, name, lambda t: re.sub(r"<shape .*</shape>", shapes, t, flags=re.S))


def triangles(cbox, name, n):
    path, _ = cbox
    obj = os.path.join(os.path.dirname(path), "meshes", name + ".obj")
    with open(obj, "w") as f:
        for i in range(n):  # unit triangles two units apart
            f.write(f"v {2 * i} 0 0\nv {2 * i + 1} 0 0\nv {2 * i} 1 0\n")
        for i in range(n):
            f.write(f"f {3 * i + 1} {3 * i + 2} {3 * i + 3}\n")
    return only_shapes(cbox, name, f'<shape type="obj"><string name="filename" value="meshes/{name}.obj"/>{DIFFUSE}</shape>')


def test_tables():
    run("tables")


def test_empty_scene(cbox):
    assert "root_kind 0, 0 primitives" in run("scene", only_shapes(cbox, "empty", "<!-- no shapes -->"), "iso=0")


def test_one_triangle(cbox):
    assert "root_kind 2, 1 primitives" in run("scene", triangles(cbox, "tri1", 1), "iso=0")


def test_two_triangles(cbox):
    # the SAH builder never splits two primitives: once as it builds them (one leaf), once under the program's
    # hand-made tree of one inner node and two leaves
    xml = triangles(cbox, "tri2", 2)
    assert "root_kind 2, 2 primitives" in run("scene", xml, "iso=0")
    assert "root_kind 1, 2 primitives, 1 inner nodes" in run("scene", xml, "iso=0", "split")


def test_cornell_box_marks_the_dielectric_sphere(cbox):
    # (the program also checks that the equally isolated mirror sphere is not marked)
    assert "1 isolated" in run("scene", cbox[0], "iso=1")


def test_sphere_touching_the_floor_is_not_isolated(cbox):
    touch = variant(cbox, "touch", lambda t: t.replace(DIELECTRIC_SPHERE, '<point name="center" value="0.4458 0.3263 0.3767"/>'))
    run("scene", touch, "iso=0")


def test_generated_mesh(tmp_path):
    xml, ntri = scenegen.bumpy_cbox_xml(str(tmp_path), 16, 12, width=64, height=64, spp=1)
    assert 300 <= ntri <= 500
    out = run("scene", xml, "iso=0")
    inner = int(re.search(r"(\d+) inner nodes", out).group(1))
    assert inner > 64  # the collapse recurses several levels, and the top sizes it checks stay below the node count


def test_nee_finite(cbox):
    diffuse = lambda t: t.replace('<bsdf type="dielectric"/>', DIFFUSE)
    run("scene", variant(cbox, "nee_diffuse", diffuse), "iso=0", "nee=1")
    point = '<emitter type="point"><point name="position" value="0 1 0"/><color name="power" value="10 10 10"/></emitter>'
    run("scene", variant(cbox, "nee_point", lambda t: diffuse(t).replace("</scene>", point + "\n</scene>")), "nee=0")
    # the mirror sphere moved up into the light mesh's box
    lifted = lambda t: diffuse(t).replace(MIRROR_SPHERE, '<point name="center" value="-0.2 1.4 -0.1"/>')
    run("scene", variant(cbox, "nee_overlap", lifted), "nee=0")
