"""Lighting graph — host mirror of the fork's src/graph tools: the
precompute and the render that consumes it.

The reference builds a "free graph" of scatter points in a medium lit by one distant light,
then solves light transport on it (cmd/graph_maker.cpp:70-160):

  FreeGraphBuilder::BuildGraph  (free/free_graph_builder.cpp:143-214) — a dimensionSteps²
      grid of rays along the light direction, `iterationsPerStep` delta-tracking walks each
      (TracePath, :19-141), scatter points merged into vertices of radius
      GetSameSpotRadius * radiusModifier (util.h:465-467);
  LightingCalculator            (lighting_calculator.cpp) — the initial light of every vertex
      by ratio tracking from a disk of rays (GetLightVector, :84-155), the transport matrix
      (GetTransportMatrix, :61-82) and the bounce iteration (ComputeFinalLight, :23-59).

Here the walks (k_graph_walks), the per-vertex transmittance estimates (k_graph_disk /
k_graph_tr / k_graph_average) and the sparse bounce iteration (k_graph_spmv) run on the GPU
through include/avr.h; the order-dependent vertex merge runs in C++ on the host
(avr_graph_add_walks) or, with FreeGraphBuilder(merge="device"), as data-parallel rounds on the
GPU followed by a host replay (k_graph_merge_round, avr_graph_add_walks_device): the same
graph. Names, parameters and error behaviour follow the reference. All
geometry is in the scene's render space; the medium's boundary primitive is its bounds box
or, with primitive="interface", the scene's interface sphere or mesh:
MediumData(scene, primitive) carries the choice, and FreeGraphBuilder, LightingCalculator,
GraphIntegrator and IntegrationAnalyzer set it on their context (capi.Context.set_graph_geometry).

ReinforceSparseVertices (:280-475) runs its rays and walks on the GPU and its sparse-vertex
checks on the host graph.

The render is GraphIntegrator (graph_integrator.cpp:180-280, free-graph branch):
FreeGraph.index(light_scalar) builds the vertex index (a cell grid, capi.GraphIndex; host
C++), and GraphIntegrator renders with it on the GPU: per camera sample the first real
scatter in the medium is connected to the vertices within the vertex radius (or, with
renderSearchRange active, within their search ranges), weighted by inverse squared distance
(k_graph_render). build_graph -> LightingCalculator.compute_final_light -> index ->
GraphIntegrator.render is the whole pipeline; the graph is handed over in memory, or through
a file in the reference's format (FreeGraph.save, load_index, GraphIntegrator.from_file;
graph_io.py), which the fork's graph_maker and `pbrt --graph` write and read too.

ComputeSearchRanges (:473-548) has three forms: compute_search_ranges (a float64 k-d tree,
the default), and compute_search_ranges_host / _device, which follow the reference's float
arithmetic and order over the vertex index (k_graph_knn, k_graph_range_average on the GPU).

IntegrationAnalyzer (graph/analysis/integration_analyzer.cpp, the fork's "analyzer"
integrator) tells whether a graph serves a camera: the camera paths are followed for maxdepth
real scatters and each scatter point is looked up in the vertex index (k_graph_analyze,
capi.GraphIndex.coverage): a vertex within the vertex radius? vertices within their own search
range, and how far? GraphAnalysis holds the per-pixel counters and the reference's figures.

The uniform graph (UniformGraph, graph.h:195; GraphIntegrator's uniform branch,
graph_integrator.cpp:89-178) has its vertices on the integer lattice of a spacing:
FreeGraph.to_uniform(spacing, light_scalar) converts a lit free graph (FreeGraph::ToUniform's
vertex part), UniformGraph.save / load_uniform go through the reference's file format, and
GraphIntegrator renders from it when handed a capi.GraphUniform: the scatter point's voxel is
looked up in one hash table (k_graph_render_uniform), with no radius search; voxel_view=True is
--graph-debug's view of the lit voxels.

The voxel boundary (VoxelBoundary, voxels/voxel_boundary.cpp) makes a uniform graph straight
from the medium: ray bundles from a sphere of points capture where the majorant grid first is
not empty (k_graph_capture), the points go onto the lattice (k_graph_uniform_insert), one flood
thins them to a single layer and another fills the inside (k_graph_voxels_level, or the same
cell rules on the host).
"""
import json
import math
import time

import numpy as np

from . import capi, graph_io
from .integrator import FilmIntegrator
from .scene import GBufferFilm

f32 = np.float32


# ---------------------------------------------------------------------------
# Config (util.h:707-748 and its from_json readers :750-812)

class GraphBuilderConfig:
    def __init__(self, radius_modifier=1.0, max_depth=100, dimension_steps=10, iterations_per_step=10,
                 render_search_range=None, edge_reinforcement=None, neighbour_reinforcement=None):
        self.radius_modifier = float(radius_modifier)
        self.max_depth = int(max_depth)
        self.dimension_steps = int(dimension_steps)
        self.iterations_per_step = int(iterations_per_step)
        self.render_search_range = render_search_range or {"active": False, "neighboursToUse": 0}
        self.edge_reinforcement = edge_reinforcement or {"active": False}
        self.neighbour_reinforcement = neighbour_reinforcement or {"active": False}


class LightingCalculatorConfig:
    def __init__(self, light_iterations=16, points_on_radius_light=2, bounces=(10,)):
        self.light_iterations = int(light_iterations)
        self.points_on_radius_light = int(points_on_radius_light)
        self.bounces = [int(b) for b in bounces]


class Config:
    def __init__(self, graph_builder=None, lighting_calculator=None):
        self.graph_builder = graph_builder or GraphBuilderConfig()
        self.lighting_calculator = lighting_calculator or LightingCalculatorConfig()

    @classmethod
    def from_json(cls, text_or_dict):
        """The reference's graph config JSON (util.h:750-812 field names)."""
        j = json.loads(text_or_dict) if isinstance(text_or_dict, str) else text_or_dict
        gb, lc = j["graphBuilder"], j["lightingCalculator"]
        b = GraphBuilderConfig(gb["radiusModifier"], gb["maxDepth"], gb["dimensionSteps"], gb["iterationsPerStep"],
                               gb["renderSearchRange"], gb.get("edgeReinforcement"), gb.get("neighbourReinforcement"))
        c = LightingCalculatorConfig(lc["lightIterations"], lc["pointsOnRadiusLight"], lc["bounces"])
        return cls(b, c)


def disk_points_size(n):
    """util::GetDiskPointsSize (util.h:206-208): points of GetDiskPoints(radius 1)."""
    if n == 0:
        return 1
    step = f32(1) / f32(n + 1)
    k = 0
    for x in range(-n, n + 1):
        for y in range(-n, n + 1):
            # CoordinateSystem((1,0,0)) = (0,0,-1), (0,1,0): |p - c| = step * sqrt(x^2 + y^2)
            a, b = f32(f32(x) * step), f32(f32(y) * step)
            if f32(np.sqrt(f32(f32(a * a) + f32(b * b)))) <= f32(1):
                k += 1
    return k


def round_up_pow2(v):
    v = int(v)
    return 1 if v <= 1 else 1 << (v - 1).bit_length()


class GraphSampling:
    """The graph tools' sampler setup (graph_maker.cpp:84-104): pixelSamples =
    RoundUpPow2(lightIterations), a square sampling resolution large enough for one sample
    index per ray, the scene's sampler type and seed."""

    def __init__(self, sampler=0, seed=0, samples_per_pixel=16, resolution=(1024, 1024)):
        self.sampler, self.seed, self.samples_per_pixel = int(sampler), int(seed), int(samples_per_pixel)
        self.resolution = (int(resolution[0]), int(resolution[1]))

    @classmethod
    def for_config(cls, config, sampler=0, seed=0):
        gb, lc = config.graph_builder, config.lighting_calculator
        max_disk = disk_points_size(lc.points_on_radius_light)
        max_sphere = max(int(gb.edge_reinforcement.get("reinforcementRays", 0)),
                         int(gb.neighbour_reinforcement.get("reinforcementRays", 0)))
        max_rays_per_vertex = max(max_disk, max_sphere)
        max_vertices = gb.dimension_steps ** 2 * gb.iterations_per_step * gb.max_depth
        dim = int(math.ceil(math.sqrt(max_vertices * max_rays_per_vertex)))
        if dim > 2 ** 31 - 1:
            raise ValueError("Dimension size too big")
        return cls(sampler, seed, round_up_pow2(lc.light_iterations), (dim, dim))

    def struct(self):
        return capi.AvrGraphSampling(self.sampler, self.seed, self.samples_per_pixel, self.resolution[0],
                                     self.resolution[1], self.resolution[0])


# ---------------------------------------------------------------------------
# Medium geometry (util.h:45-91 PrimitiveData / MediumData, 419-503 GetHits / StartEndT)

def _gamma(n):
    eps = f32(np.finfo(np.float32).eps) * f32(0.5)
    return f32(f32(n) * eps) / f32(f32(1) - f32(f32(n) * eps))


def _xf_point(m, p):   # Transform::operator()(Point3f): left-to-right sums (affine)
    return np.array([f32(f32(f32(m[r, 0] * p[0]) + f32(m[r, 1] * p[1])) + f32(m[r, 2] * p[2])) + m[r, 3]
                     for r in range(3)], f32)


def _xf_vector(m, v):
    return np.array([f32(f32(f32(m[r, 0] * v[0]) + f32(m[r, 1] * v[1])) + f32(m[r, 2] * v[2])) for r in range(3)], f32)


def coordinate_system(v):
    """CoordinateSystem (vecmath.h:1007-1013) in float32."""
    v = np.asarray(v, f32)
    sign = f32(math.copysign(1.0, float(v[2])))
    a = f32(-1) / f32(sign + v[2])
    b = f32(f32(v[0] * v[1]) * a)
    x = np.array([f32(1) + f32(f32(sign * f32(v[0] * v[0])) * a), f32(sign * b), f32(-sign * v[0])], f32)
    y = np.array([b, f32(sign + f32(f32(v[1] * v[1]) * a)), f32(-v[1])], f32)
    return x, y


PRIMITIVES = ("box", "interface")


def parse_interface_sphere(text):
    """The tools' --interface-sphere CX,CY,CZ,R (world space) as Scene's interface_sphere
    argument ((cx, cy, cz), r); ValueError unless four finite numbers with r > 0."""
    parts = [v.strip() for v in str(text).split(",")]
    if len(parts) != 4:
        raise ValueError(f"interface sphere {text!r}: expected CX,CY,CZ,R")
    cx, cy, cz, r = (float(v) for v in parts)
    if not all(math.isfinite(v) for v in (cx, cy, cz, r)) or not r > 0:
        raise ValueError(f"interface sphere {text!r}: finite centre and a radius > 0 required")
    return (cx, cy, cz), r


def _check_primitive(primitive):
    if primitive not in PRIMITIVES:
        raise ValueError('primitive must be "box" or "interface"')
    return primitive


class MediumData:
    """util::MediumData / PrimitiveData (util.h:45-91): the bounds of the medium's boundary
    primitive in render space (pmin, pmax), their center and maxDistToCenter = |Diagonal / 2|.
    primitive="box": the medium's bounds box. primitive="interface": the scene's interface, as
    the reference takes the scene's primitive: the sphere's bounds c -+ r (Sphere::Bounds of a
    translated sphere) or the bounds of the mesh's vertices; the box when the scene has no
    interface. `geometry` is the value avr_graph_set_geometry takes (0 box, 1 interface)."""

    def __init__(self, scene, primitive="box"):
        med = scene.medium
        self.scene = scene
        self.primitive = _check_primitive(primitive)
        self.geometry = capi.GRAPH_GEOMETRY[primitive]
        self.mfr = np.asarray(scene.medium_from_render, f32)
        b = np.asarray(med.bounds, f32)
        self.bmin, self.bmax = b[:3], b[3:]
        rfm = np.asarray(scene.render_from_medium, f32)
        corners = [_xf_point(rfm, np.array([x, y, z], f32)) for x in (b[0], b[3]) for y in (b[1], b[4])
                   for z in (b[2], b[5])]
        self.pmin = np.min(corners, axis=0).astype(f32)
        self.pmax = np.max(corners, axis=0).astype(f32)
        sph = getattr(scene, "interface_sphere_render", None)
        verts = getattr(scene, "interface_vertices_render", None)
        # what the device intersects (primitive_hits): the sphere, the mesh's planes, or the box
        self.shape = "box"
        if primitive == "interface" and sph is not None:
            c, r = np.asarray(sph[:3], f32), f32(sph[3])
            self.pmin, self.pmax = (c - r).astype(f32), (c + r).astype(f32)
            self.shape = "sphere"
        elif primitive == "interface" and verts is not None:
            v = np.asarray(verts, f32).reshape(-1, 3)
            self.pmin, self.pmax = v.min(axis=0).astype(f32), v.max(axis=0).astype(f32)
            self.shape = "mesh"
        diag = (self.pmax - self.pmin).astype(f32)
        half = (diag / f32(2)).astype(f32)
        self.bounds_center = (self.pmin + half).astype(f32)
        self.max_dist_to_center = f32(np.sqrt(f32(f32(f32(half[0] * half[0]) + f32(half[1] * half[1])) +
                                                  f32(half[2] * half[2]))))

    def box_hits(self, o, d):
        """GetHits(primitive) in the model: (type, t0, t1); 0 OutsideTwoHits, 2 zero hits,
        3 InsideOneHit (t0 = exit). Bounds3::IntersectP (vecmath.h:1547-1571) in medium space."""
        om, dm = _xf_point(self.mfr, o), _xf_vector(self.mfr, d)
        t0, t1 = f32(0), f32(np.inf)
        s = f32(f32(1) + f32(f32(2) * _gamma(3)))
        with np.errstate(divide="ignore", invalid="ignore"):
            for i in range(3):
                inv = f32(f32(1) / dm[i])
                tn = f32(f32(self.bmin[i] - om[i]) * inv)
                tf = f32(f32(self.bmax[i] - om[i]) * inv)
                if tn > tf:
                    tn, tf = tf, tn
                tf = f32(tf * s)
                t0 = tn if tn > t0 else t0
                t1 = tf if tf < t1 else t1
                if t0 > t1:
                    return 2, f32(0), f32(0)
        if t0 > 0:
            return 0, t0, t1
        return 3, t1, f32(0)


def same_spot_radius(medium_data):
    """GetSameSpotRadius (util.h:465-467)."""
    return f32(f32(medium_data.max_dist_to_center * f32(2)) / f32(1000))


# ---------------------------------------------------------------------------

class FreeGraph:
    """The assembled graph: vertices (id = row), vertex samples, edges with samples, and
    the in-node path length average (Graph::inNodePathLengthAverager)."""

    def __init__(self, builder_handle, radius):
        self._g = builder_handle
        self.radius = f32(radius)
        self.points, self.samples = builder_handle.vertices()
        self.edge_from, self.edge_to, self.edge_samples = builder_handle.edges()
        self.in_node_path_length, self.in_node_path_count = builder_handle.in_node_path_length()
        self.search_range = None

    @property
    def num_vertices(self):
        return len(self.samples)

    def transport_csr(self):
        """GetTransportMatrix (lighting_calculator.cpp:61-82) as CSR."""
        return self._g.transport()

    def index(self, light_scalar):
        """The render's vertex index (GraphIntegrator::Initialize): these vertices with
        `light_scalar` (LightingCalculator.light_scalar) as VertexData::lightScalar, the
        vertex radius, and the search ranges when the builder computed them
        (useRenderSearchRange)."""
        return capi.GraphIndex(self.points, light_scalar, self.search_range, radius=self.radius)

    def save(self, path, light_scalar, description="basic", precision=9, edges=False):
        """Graph::WriteToDisk as graph_maker calls it (graph_io.write_graph): the vertices with
        `light_scalar` and, when computed, their search ranges, in the reference's file format."""
        graph_io.write_graph(path, self, light_scalar, description=description, precision=precision, edges=edges)


    def to_uniform(self, spacing, light_scalar, reduce="first"):
        """FreeGraph::ToUniform (graph.cpp:597-604), the vertex part: a UniformGraph of
        `spacing` over these vertices with `light_scalar`, taken in ascending id (the reference
        iterates an unordered map: its order is unspecified); the first vertex of a voxel makes
        the new vertex. reduce "first" keeps that vertex's light, as the reference's AddVertex
        does; "mean" takes the float mean of the voxel's lights. Edges and paths are not
        carried: the render reads neither."""
        return UniformGraph(capi.GraphUniform.from_points(self.points, light_scalar, spacing, reduce=reduce))


class UniformGraph:
    """A uniform lighting graph: capi.GraphUniform (`.table`, what GraphIntegrator takes) with
    the graph-level names: spacing, coors (m, 3), points, light_scalar, num_vertices,
    vertex_of (after a conversion: old -> new vertex id), save."""

    def __init__(self, table):
        self.table = table
        self.spacing = table.spacing
        self.coors = table.coors
        self.light_scalar = table.light_scalar
        self.vertex_of = getattr(table, "vertex_of", None)

    @property
    def num_vertices(self):
        return self.table.num_vertices

    @property
    def points(self):
        return self.table.points

    def save(self, path, description="basic", precision=9):
        """UniformGraph::WriteToStream's file (graph_io.write_uniform_graph)."""
        graph_io.write_uniform_graph(path, self, description=description, precision=precision)


def load_uniform(path):
    """The uniform graph of a graph file (UniformGraph::ReadFromDisk): the vertices are added
    in file order, keyed by FitToGraph(point); a later vertex in an occupied voxel is dropped,
    as ReadFromStream -> AddVertex does (the coors column is read but is not the key). Vertex
    ids are the order of first appearance. Raises on a free graph and on a file written
    without lighting."""
    g = graph_io.read_graph(path)
    if g.kind != "uniform":
        raise ValueError(f"{path}: a {g.kind} graph; load_uniform takes uniform graphs")
    if g.light_scalar is None:
        raise ValueError(f"{path}: written without lighting (useLighting False): nothing to render")
    if g.num_vertices == 0:
        raise ValueError(f"{path}: no vertices")
    order = g.file_ids
    return UniformGraph(capi.GraphUniform.from_points(g.points[order], g.light_scalar[order], g.spacing, reduce="first"))


# ---------------------------------------------------------------------------
# Voxel boundary (voxels/voxel_boundary.{h,cpp})

_PI = f32(3.14159265358979323846)


def _rotate_x(deg):   # RotateX (transform.cpp:49-57), the 3x3 part
    rad = f32(f32(_PI / f32(180)) * f32(deg))
    s, c = f32(np.sin(rad)), f32(np.cos(rad))
    return np.array([[1, 0, 0, 0], [0, c, -s, 0], [0, s, c, 0]], f32)


def _spherical_direction(sin_t, cos_t, phi):   # vecmath.h:1666-1673
    st, ct = f32(min(max(sin_t, f32(-1)), f32(1))), f32(min(max(cos_t, f32(-1)), f32(1)))
    return np.array([f32(st * f32(np.cos(f32(phi)))), f32(st * f32(np.sin(f32(phi)))), ct], f32)


def sphere_surface_points(center, radius, equator_step_degrees):
    """util::GetSphereSurfacePoints (util.h:134-176) in its float operation order: rings of
    points from the equator (elevation 0) up to the pole in steps of equator_step_degrees, the
    step in phi widened by the ring's radius ratio; every elevation other than 0 gives an up
    point and a down point per phi. Returns (n, 3) float32 in the reference's order. ValueError
    unless 0 < step <= 90. sin and cos are the platform's float routines, as in the reference
    (std::sin / std::cos of a float): they are not pinned, so the last bit of a point may differ
    between platforms."""
    step = f32(equator_step_degrees)
    if not (step > 0 and step <= 90):
        raise ValueError("Step must be between 0 and 90 degrees")
    center = np.asarray(center, f32).reshape(3)
    radius = f32(radius)
    to_world = _rotate_x(-90)
    pts = []
    elevation = f32(0)
    with np.errstate(divide="ignore", over="ignore"):
        while elevation <= 90:
            rad = f32(f32(f32(f32(90) - elevation) * _PI) / f32(180))
            sin_t, cos_t = f32(np.sin(rad)), f32(np.cos(rad))
            rad_down = f32(f32(f32(f32(90) + elevation) * _PI) / f32(180))
            sin_d, cos_d = f32(np.sin(rad_down)), f32(np.cos(rad_down))
            d = _xf_vector(to_world, _spherical_direction(sin_t, cos_t, f32(0)))
            ratio = f32(np.sqrt(f32(f32(f32(d[0] * d[0]) + f32(0)) + f32(d[2] * d[2]))))
            phi_step = f32(step / ratio)
            # at least two points on a circle, except for the pole
            if phi_step >= 180 and float(ratio) > 1e-6:
                break
            phi = f32(0)
            while phi < 360:
                phi_rad = f32(f32(phi * _PI) / f32(180))
                up = _xf_vector(to_world, _spherical_direction(sin_t, cos_t, phi_rad))
                pts.append((center + (up * radius).astype(f32)).astype(f32))
                if elevation != 0:
                    down = _xf_vector(to_world, _spherical_direction(sin_d, cos_d, phi_rad))
                    pts.append((center + (down * radius).astype(f32)).astype(f32))
                phi = f32(phi + phi_step)
            elevation = f32(elevation + step)
    return np.array(pts, f32).reshape(-1, 3)


class VoxelBoundary:
    """graph::VoxelBoundary (voxels/voxel_boundary.cpp): a medium to a voxel set. Ray bundles
    shot at the medium from a sphere around it keep the first non-empty majorant cell they meet
    (capture_points, k_graph_capture); the points go onto the lattice of a spacing and a flood
    from outside thins them to the voxels that touch the outside (capture_boundary); a flood
    from that boundary fills the inside (fill_inside). Every result is a UniformGraph with
    lights 0; the filled one's points, lit by Context.graph_light, make a uniform lighting graph
    straight from the medium, with no walks and no merge.

    Bundles (CaptureBoundary :15-31): origin = a point of sphere_surface_points(bounds_center,
    2 max_dist_to_center, equator_step); dir = bounds_center - origin, not normalised;
    (xv, yv) = CoordinateSystem(dir) * (max_dist_to_center / num_steps); (2 num_steps + 1)^2 rays
    per bundle. frame="reference" hands CoordinateSystem the un-normalised dir, as the reference
    does: the function assumes a unit vector, so the frame is skewed and not of unit length.
    frame="orthonormal", a deviation, builds the frame from normalize(dir); the rays still run
    along dir itself. num_steps is the reference's constant 100.

    device=False runs the conversion and the floods on the host (the capture itself is device
    code); ctx may then be None when points are handed to capture_boundary."""

    def __init__(self, ctx, medium_data, num_steps=100, frame="reference", device=True):
        if frame not in ("reference", "orthonormal"):
            raise ValueError('frame must be "reference" or "orthonormal"')
        if int(num_steps) < 1:
            raise ValueError("num_steps must be at least 1")
        self.ctx = ctx
        self.md = medium_data
        self.num_steps = int(num_steps)
        self.frame = frame
        self.device = bool(device)
        self.seconds = {}
        if ctx is not None and getattr(medium_data, "geometry", None) is not None:
            ctx.set_graph_geometry(medium_data.geometry)

    def bundles(self, equator_step=10.0):
        """(origin, dir, xv, yv), (n, 3) float32 each: one bundle per sphere point."""
        md = self.md
        ctr = np.asarray(md.bounds_center, f32)
        origins = sphere_surface_points(ctr, f32(md.max_dist_to_center * f32(2)), equator_step)
        step = f32(md.max_dist_to_center / f32(self.num_steps))
        dirs, xs, ys = [], [], []
        for o in origins:
            d = (ctr - o).astype(f32)
            basis = d
            if self.frame == "orthonormal":
                ln = f32(np.sqrt(f32(f32(f32(d[0] * d[0]) + f32(d[1] * d[1])) + f32(d[2] * d[2]))))
                basis = (d / ln).astype(f32)
            xv, yv = coordinate_system(basis)
            dirs.append(d)
            xs.append((xv * step).astype(f32))
            ys.append((yv * step).astype(f32))
        return origins, np.array(dirs, f32), np.array(xs, f32), np.array(ys, f32)

    def capture_points(self, equator_step=10.0):
        """CaptureBoundary(equatorStepSize) (:13-62): the captured points, (k, 3) float32 in ray
        order (bundle, i, j). last_rays holds the number of rays shot."""
        o, d, xv, yv = self.bundles(equator_step)
        t0 = time.perf_counter()
        pts, flag, _ = self.ctx.graph_capture(o, d, xv, yv, self.num_steps)
        self.seconds["capture"] = time.perf_counter() - t0
        self.last_rays = len(flag)
        return np.ascontiguousarray(pts[flag])

    def _count(self, points, spacing):
        if self.device:
            return self.ctx.graph_uniform_count(points, spacing)
        return capi.GraphUniform.from_points(points, np.zeros(len(points), f32), spacing).num_vertices

    def _to_uniform(self, points, spacing):
        if self.device:
            return capi.GraphUniform.from_points_device(self.ctx, points, spacing)
        return capi.GraphUniform.from_points(points, np.zeros(len(points), f32), spacing)

    def bisect_spacing(self, points, wanted_vertices, count=None):
        """CaptureBoundary(wantedVertices)'s search (:64-91) in float32: spacingGTE1 = count(1)
        >= wanted; ten steps of middle = min + (max - min) / 2 over [1, 1000], the spacing tried
        middle / (spacingGTE1 ? 1 : 1000); count > wanted moves min, else max. Returns every
        spacing tried in order; the last is the graph's."""
        count = count or (lambda s: self._count(points, s))
        wanted = int(wanted_vertices)
        gte1 = count(f32(1)) >= wanted
        lo, hi, tried = f32(1), f32(1000), []
        for _ in range(10):
            middle = f32(lo + f32(f32(hi - lo) / f32(2)))
            spacing = f32(middle / (f32(1) if gte1 else f32(1000)))
            tried.append(spacing)
            if count(spacing) > wanted:
                lo = middle
            else:
                hi = middle
        return tried

    def capture_boundary(self, spacing=None, wanted_vertices=None, equator_step=10.0, points=None):
        """CaptureBoundary(spacing, equatorStepSize) (:97-104) or CaptureBoundary(wantedVertices,
        equatorStepSize) (:64-95): the captured points (or `points`) on the lattice of the
        spacing, thinned to a single layer. The UniformGraph returned holds the surviving
        vertices in ascending old id, renumbered from 0; old_to_new maps every vertex of the
        unthinned graph to its new id or -1, old_ids back; visited is the reference's numVisited,
        num_captured the vertices before thinning, spacings_tried the bisection's."""
        if (spacing is None) == (wanted_vertices is None):
            raise ValueError("capture_boundary: exactly one of spacing and wanted_vertices")
        if points is None:
            points = self.capture_points(equator_step)
        points = np.ascontiguousarray(points, f32).reshape(-1, 3)
        tried = None
        t0 = time.perf_counter()
        if spacing is None:
            tried = self.bisect_spacing(points, wanted_vertices)
            spacing = tried[-1]
        full = self._to_uniform(points, f32(spacing))
        self.seconds["to_uniform"] = time.perf_counter() - t0
        g = self.to_single_layer(UniformGraph(full))
        g.spacings_tried = tried
        return g

    def to_single_layer(self, graph):
        """ToSingleLayerAndSaveCast (:122-181) on a UniformGraph: a new graph of the vertices that
        touch the outside; the flood's state (the cast set) stays with it for fill_inside."""
        md = self.md
        vox = capi.GraphVoxels(md.pmin, md.pmax, graph.spacing, graph.coors)
        t0 = time.perf_counter()
        levels = vox.single_layer(self.ctx if self.device else None)
        self.seconds["single_layer"] = time.perf_counter() - t0
        keep = (vox.vertex_bits() & capi.VOXEL_SINGLE) != 0
        old_ids = np.nonzero(keep)[0].astype(np.int32)
        if len(old_ids) == 0:
            raise ValueError("single layer: no vertex touches the outside")
        old_to_new = np.full(len(keep), -1, np.int32)
        old_to_new[old_ids] = np.arange(len(old_ids), dtype=np.int32)
        g = UniformGraph(capi.GraphUniform(graph.coors[old_ids], np.zeros(len(old_ids), f32), graph.spacing))
        g.old_to_new, g.old_ids = old_to_new, old_ids
        g.num_captured = graph.num_vertices
        g.visited, g.levels = vox.counts()[0], levels
        g.spacings_tried = None
        g.voxels = vox
        return g

    def fill_inside(self, boundary, start=None):
        """FillInside (:183-225): a UniformGraph of every cell a 6-neighbour flood reaches from
        the boundary without entering a cast cell. start: a vertex id of `boundary`; None takes
        the lowest, "all" floods from every vertex, which also fills several disjoint blobs. The
        reference starts from unordered_map::begin(), which is unspecified, and numbers the
        filled vertices in the flood's FIFO order from there; here the ids run in ascending
        (z, y, x). A graph that has not been through to_single_layer goes through it first
        (:184-186); start is then one of its own ids that survives."""
        vox = getattr(boundary, "voxels", None) if hasattr(boundary, "old_ids") else None
        s = start
        if vox is None:
            vox = self.to_single_layer(boundary).voxels
        elif start is not None and start != "all" and start != "lowest":
            if isinstance(start, bool) or not isinstance(start, (int, np.integer)) or not 0 <= start < len(boundary.old_ids):
                raise ValueError(f"fill_inside: start {start!r} is no vertex of the boundary")
            s = int(boundary.old_ids[start])
        t0 = time.perf_counter()
        levels = vox.fill(self.ctx if self.device else None, s)
        self.seconds["fill"] = time.perf_counter() - t0
        coors = vox.cells_with(capi.VOXEL_FILLED)
        g = UniformGraph(capi.GraphUniform(coors, np.zeros(len(coors), f32), boundary.spacing))
        g.levels = levels
        g.voxels = vox
        return g


def load_index(path):
    """The render's vertex index from a graph file (FreeGraph::ReadFromDisk followed by
    GraphIntegrator::Initialize): its points, lightScalar, renderSearchRange where present, and
    vertex radius. Raises on a uniform graph and on a file written without lighting."""
    g = graph_io.read_graph(path)
    if g.kind != "free":
        raise ValueError(f"{path}: a {g.kind} graph; the render takes free graphs")
    if g.light_scalar is None:
        raise ValueError(f"{path}: written without lighting (useLighting False): nothing to render")
    if g.num_vertices == 0:
        raise ValueError(f"{path}: no vertices")
    return capi.GraphIndex(g.points, g.light_scalar, g.search_range, radius=g.radius)


class FreeGraphBuilder:
    """FreeGraphBuilder (free/free_graph_builder.cpp): walks on the GPU, merge on the host or,
    with merge="device", in rounds on the GPU (the same graph)."""

    def __init__(self, ctx, medium_data, in_direction, sampling, config, node_radius=None, sample_index_offset=0,
                 search_ranges="scipy", merge="host"):
        """search_ranges: how ComputeSearchRanges runs: "scipy" (compute_search_ranges, the
        float64 k-d tree), "host" or "device" (compute_search_ranges_host / _device: the
        reference's float arithmetic over the vertex index; the two agree bitwise).
        merge: how the walks' scatter points become vertices, in build_graph and in every
        reinforcement cycle: "host" (avr_graph_add_walks, in walk order) or "device"
        (avr_graph_add_walks_device: the assignment in rounds on the GPU, then the host replay;
        the same graph). merge_stats holds the last device merge's avr_graph_merge_stats,
        merge_seconds and merge_rounds the sums over this builder's merge calls."""
        if search_ranges not in ("scipy", "host", "device"):
            raise ValueError('search_ranges must be "scipy", "host" or "device"')
        if merge not in ("host", "device"):
            raise ValueError('merge must be "host" or "device"')
        self.search_ranges = search_ranges
        self.merge = merge
        self.merge_stats = None
        self.merge_seconds = 0.0
        self.merge_rounds = 0
        self.ctx = ctx
        self.md = medium_data
        self.in_dir = np.asarray(in_direction, f32)
        self.sampling = sampling
        self.config = config
        r = node_radius if node_radius is not None else f32(same_spot_radius(medium_data) * f32(config.radius_modifier))
        self.radius = f32(r)
        self.sample_index_offset = int(sample_index_offset)
        if ctx is not None and medium_data is not None:
            ctx.set_graph_geometry(medium_data.geometry)

    def _start_rays_device(self):
        c, md, d = self.config, self.md, self.in_dir
        ty, o, t = self.ctx.graph_start_rays(md.bounds_center, md.max_dist_to_center, d, c.dimension_steps)
        sel = ty != 2
        idx = np.arange(c.dimension_steps ** 2, dtype=np.int64)[sel] * c.iterations_per_step
        n = int(sel.sum())
        return o[sel].reshape(n, 3), np.tile(d, (n, 1)).astype(f32), t[sel], idx

    def grid_points(self):
        """The ray grid's points before the primitive's crossing, (dimension_steps^2, 3) float32
        in the loop's order (x outer): BuildGraph :143-165 in its float operation order, from
        the primitive's bounds_center and max_dist_to_center."""
        c, md, d = self.config, self.md, self.in_dir
        xv, yv = coordinate_system(d)
        origin = (md.bounds_center - (d * md.max_dist_to_center) * f32(2)).astype(f32)
        origin = (origin - ((xv + yv).astype(f32) * md.max_dist_to_center)).astype(f32)
        step = f32(f32(md.max_dist_to_center * f32(2)) / f32(c.dimension_steps + 1))
        xv, yv = (xv * step).astype(f32), (yv * step).astype(f32)
        return np.array([((origin + (xv * f32(x)).astype(f32)).astype(f32) + (yv * f32(y)).astype(f32)).astype(f32)
                         for x in range(1, c.dimension_steps + 1) for y in range(1, c.dimension_steps + 1)],
                        f32).reshape(-1, 3)

    def start_rays(self, device=None):
        """BuildGraph's ray grid (:143-199): origins, directions, first-segment tMax (the
        primitive's exit after SkipIntersection) and the first sampling index per ray.
        device=True runs the grid on the GPU (avr_graph_start_rays; for the box bitwise the
        host loop), which an interface sphere or mesh always does (device=False raises there)."""
        c = self.config
        md = self.md
        d = self.in_dir
        if device is None:
            device = md.shape != "box"
        if device:
            return self._start_rays_device()
        if md.shape != "box":
            raise ValueError("the ray grid of an interface primitive runs on the device (start_rays(device=True))")
        grid = self.grid_points()
        o, t, idx = [], [], []
        for x in range(1, c.dimension_steps + 1):
            for y in range(1, c.dimension_steps + 1):
                p = grid[(y - 1) + (x - 1) * c.dimension_steps]
                ty, t0, t1 = md.box_hits(p, d)
                if ty == 2:
                    continue
                if ty == 0:
                    p = (p + (d * t0).astype(f32)).astype(f32)     # SkipIntersection (no offset)
                    t_exit = f32(t1 - t0)
                else:
                    t_exit = t0
                o.append(p)
                t.append(t_exit)
                idx.append(((y - 1) + (x - 1) * c.dimension_steps) * c.iterations_per_step)
        n = len(o)
        return (np.array(o, f32).reshape(n, 3), np.tile(d, (n, 1)).astype(f32), np.array(t, f32),
                np.array(idx, np.int64))

    def build_graph(self, search_ranges=True):
        """BuildGraph (:143-214). search_ranges=False leaves ComputeSearchRanges to a later
        compute_search_ranges(graph) call (tools/graph_maker.py times the two apart)."""
        c = self.config
        o, d, t, idx = self.start_rays()
        pts, counts = self.ctx.graph_walks(self.sampling.struct(), o, d, t, idx, c.iterations_per_step,
                                           self.sample_index_offset, c.max_depth)
        g = capi.Graph(self.radius)
        self._add_walks(g, pts, counts, c.max_depth)
        self.reinforce_cycles = self.reinforce_sparse_vertices(g)
        graph = FreeGraph(g, self.radius)
        if search_ranges:
            self.compute_search_ranges(graph)
        return graph

    def compute_search_ranges(self, graph):
        """ComputeSearchRanges (:498-548), BuildGraph's last step: sets graph.search_range when
        renderSearchRange is active, in the form the constructor's `search_ranges` names."""
        c = self.config
        if not c.render_search_range.get("active"):
            return
        k = int(c.render_search_range["neighboursToUse"])
        if self.search_ranges == "device":
            graph.search_range = compute_search_ranges_device(self.ctx, graph.points, self.radius, k)
        elif self.search_ranges == "host":
            graph.search_range = compute_search_ranges_host(graph.points, self.radius, k)
        else:
            graph.search_range = compute_search_ranges(graph.points, k)


    def _reinforce(self, g, ids, cfg, cycle):
        """ReinforceSparseVertices(graph, sparseVertices, ...) (:434-475): every listed
        vertex's sphere rays in one device call, their walks in a second (the rays never
        depend on the graph), merged in vertex then point order as the reference's loop."""
        if not len(ids):
            return
        md = self.config.max_depth
        k = int(cfg["reinforcementRays"])
        ids = np.asarray(ids, np.int32)
        xyz, _ = g.vertices()
        smp = self.sampling.struct()
        o, d, t, valid = self.ctx.graph_reinforce_rays(smp, ids, xyz[ids], self.radius, k, cycle)
        sel = valid.ravel() != 0
        if not sel.any():
            return
        index0 = (ids.astype(np.int64)[:, None] * k + np.arange(k)[None, :]).ravel()[sel]
        pts, counts = self.ctx.graph_walks(smp, o.reshape(-1, 3)[sel], d.reshape(-1, 3)[sel], t.ravel()[sel], index0,
                                           1, cycle, md - 1, skip_dims=2)
        padded = np.zeros((len(counts), md, 3), np.float32)   # avr_graph_add_walks_from: stride max_depth
        padded[:, :md - 1] = pts[:, :md - 1]
        self._add_walks(g, padded, counts, md, np.repeat(ids, k)[sel])

    def _add_walks(self, g, pts, counts, max_depth, start_vertex=None):
        """The walks into the graph, by the builder's merge form."""
        t0 = time.perf_counter()
        if self.merge == "device":
            self.merge_stats = g.add_walks_device(self.ctx, pts, counts, max_depth, start_vertex)
            self.merge_rounds += self.merge_stats["rounds"]
        elif start_vertex is None:
            g.add_walks(pts, counts, max_depth)
        else:
            g.add_walks_from(pts, counts, max_depth, start_vertex)
        self.merge_seconds += time.perf_counter() - t0

    def reinforce_sparse_vertices(self, g):
        """FreeGraphBuilder::ReinforceSparseVertices (free_graph_builder.cpp:280-432): until the
        fraction of initial vertices with fewer than `edgesForNotSparse` out-edges (and / or
        fewer than `neighboursForNotSparse` vertices within radius x neighbourRangeModifier)
        drops below `unsatisfiedAllowedRatio`, walks from `reinforcementRays` random points in
        each sparse vertex's sphere are added, one sampler cycle per round. The sparse lists are
        re-checked after every pass (the reference skips the re-check when quiet, :392-408,
        which never terminates). Returns the cycles run."""
        c = self.config
        ec, nc = c.edge_reinforcement, c.neighbour_reinforcement
        ea, na = bool(ec.get("active")), bool(nc.get("active"))
        if not (ea or na):
            return 0
        if c.max_depth == 1:
            raise ValueError("Unable to reinforce with max depth of 1")
        n0 = g.size()[0]
        initial = np.arange(n0, dtype=np.int32)
        r_sq = f32(self.radius * self.radius)
        n_radius = f32(f32(np.sqrt(r_sq)) * f32(nc.get("neighbourRangeModifier", 1.0)))
        state = {"e": initial, "n": initial}

        def check_e():
            deg = g.out_degrees()
            state["e"] = state["e"][deg[state["e"]] < int(ec["edgesForNotSparse"])]
            return len(state["e"]) / n0 < float(ec["unsatisfiedAllowedRatio"])

        def check_n():
            cnt = g.count_in_radius(state["n"], n_radius)
            state["n"] = state["n"][cnt < int(nc["neighboursForNotSparse"])]
            return len(state["n"]) / n0 < float(nc["unsatisfiedAllowedRatio"])

        sat_e = check_e() if ea else True
        sat_n = check_n() if na else True
        cycle = 0
        while not (sat_e and sat_n):
            if cycle >= self.max_reinforce_cycles:
                raise RuntimeError(f"graph reinforcement not satisfied after {cycle} cycles")
            if ea and not sat_e:
                self._reinforce(g, state["e"], ec, cycle)
                sat_e = check_e()
            if na and not sat_n:
                self._reinforce(g, state["n"], nc, cycle)
                sat_n = check_n()
            cycle += 1
        return cycle

    max_reinforce_cycles = 64


def _search_range_index(points, radius, n_closest):
    points = np.ascontiguousarray(points, f32).reshape(-1, 3)
    if n_closest > len(points):
        raise ValueError("Graph does not contain enough vertices")
    return capi.GraphIndex(points, np.zeros(len(points), f32), None, radius=radius)


def compute_search_ranges_host(points, radius, n_closest):
    """FreeGraphBuilder::ComputeSearchRanges (:473-548) in the reference's float arithmetic
    and order, on the host: a vertex index over `points` (cell edge from `radius`, the vertex
    radius; zero light) and avr_graph_index_search_ranges. n_closest <= min(15, n - 1)."""
    idx = _search_range_index(points, radius, n_closest)
    try:
        return idx.search_ranges(int(n_closest))
    finally:
        idx.close()


def compute_search_ranges_device(ctx, points, radius, n_closest):
    """compute_search_ranges_host on the GPU (k_graph_knn, k_graph_range_average), with
    bitwise its values."""
    idx = _search_range_index(points, radius, n_closest)
    try:
        return ctx.graph_search_ranges(idx, int(n_closest))
    finally:
        idx.close()


def compute_search_ranges(points, n_closest):
    """FreeGraphBuilder::ComputeSearchRanges (:486-548): the average distance to the
    n closest other vertices, averaged again over the vertex and those neighbours. The
    legacy form: a float64 k-d tree query with numpy means (compute_search_ranges_host /
    _device follow the reference's float arithmetic and order)."""
    n = len(points)
    if n_closest > n:
        raise ValueError("Graph does not contain enough vertices")
    from scipy.spatial import cKDTree
    tree = cKDTree(points.astype(np.float64))
    dist, nb = tree.query(points.astype(np.float64), k=min(n, n_closest + 1))
    dist, nb = np.atleast_2d(dist)[:, 1:], np.atleast_2d(nb)[:, 1:]
    avg = dist.mean(axis=1).astype(f32) if n_closest > 0 else np.zeros(n, f32)
    return ((avg + avg[nb].sum(axis=1)) / (1 + nb.shape[1])).astype(f32)


class LightingCalculator:
    """LightingCalculator (lighting_calculator.cpp): light vector and bounce propagation
    on the GPU."""

    def __init__(self, ctx, graph, medium_data, in_direction, sampling, config, primitive=None):
        """primitive: None takes `medium_data`'s; "box" or "interface" must agree with it
        (max_dist_to_center is that primitive's)."""
        if config.light_iterations <= 0:
            raise ValueError("Must have at least one light ray iteration")
        if primitive is not None and _check_primitive(primitive) != medium_data.primitive:
            raise ValueError(f'primitive "{primitive}" differs from the MediumData\'s "{medium_data.primitive}"')
        self.ctx, self.graph, self.md = ctx, graph, medium_data
        self.in_dir = np.asarray(in_direction, f32)
        self.sampling, self.config = sampling, config
        self.light_scalar = None

    def get_light_vector(self):
        c = self.config
        self.ctx.set_graph_geometry(self.md.geometry)
        return self.ctx.graph_light(self.sampling.struct(), self.graph.points, self.in_dir, self.graph.radius,
                                    c.points_on_radius_light, c.light_iterations, self.md.max_dist_to_center)

    def get_transport_matrix(self):
        return self.graph.transport_csr()

    def compute_final_light(self, bounces_index=0, light=None, transport=None):
        """Returns the bounces completed; sets light_scalar (VertexData.lightScalar)."""
        light = self.get_light_vector() if light is None else light
        rp, col, val = self.get_transport_matrix() if transport is None else transport
        total, it = self.ctx.graph_propagate(rp, col, val, light, self.config.bounces[bounces_index])
        self.light_scalar = total
        return it


# ---------------------------------------------------------------------------
# The render (graph_integrator.cpp)

class GraphIntegrator(FilmIntegrator):
    """GraphIntegrator, free-graph branch (graph_integrator.cpp:180-280): every camera ray's
    first real scatter point in the medium is connected to the graph vertices around it
    (k_graph_render, avr_graph_render), which gives the graph's multiple scattering at about
    the cost of single scattering. `graph_index` is FreeGraph.index(light_scalar) or a
    capi.GraphIndex over any vertices. `graph_from_render` (4x4, affine) maps a render-space
    scatter point into the graph's space: the identity by default, since the graph tools here
    work in the scene's render space; a graph made in world space, as the reference's
    graph_maker makes them, takes inv(scene.render_from_world). `primitive` is the geometry
    model's primitive, which should be the one the graph was made with: "box" (the default), the
    medium's bounds box, which refuses a scene with an interface sphere or mesh; "interface",
    the scene's interface sphere or mesh (the box for a scene without one). The scene needs
    exactly one DistantLight and not a GBufferFilm (its geometric channels have no meaning
    here). A capi.GraphUniform (or a UniformGraph) as `graph_index` renders the uniform branch
    (:89-178) instead: L = lightSpectrum * lightScalar * light_scale for the vertex of the
    scatter point's voxel (k_graph_render_uniform); light_scale is the reference's Inv4Pi by
    default, and a graph whose light comes from LightingCalculator, which already carries
    Inv4Pi, takes light_scale=1. voxel_view=True is --graph-debug (:104-131): every camera ray
    shows the first lit voxel it enters, without light_scale. render(), film_sums(), image(), get_image() and write_image() are
    VolPathIntegrator's."""

    def __init__(self, scene, graph_index, spp=1, seed=0, graph_from_render=None, device=0, max_paths=0,
                 primitive="box", voxel_view=False, light_scale=None):
        if isinstance(scene.film, GBufferFilm):
            raise ValueError("GraphIntegrator does not render into a GBufferFilm")
        self.primitive = _check_primitive(primitive)
        self.scene = scene
        self.index = graph_index.table if isinstance(graph_index, UniformGraph) else graph_index
        self.voxel_view = bool(voxel_view)
        self.light_scale = capi.INV_4PI if light_scale is None else float(light_scale)
        self.spp = int(spp)
        self.seed = int(seed)
        self.device = int(device)
        self.graph_from_render = None if graph_from_render is None else np.asarray(graph_from_render, f32).reshape(4, 4)
        self.ctx = capi.Context(device, max_paths)
        self.ctx.set_scene(scene)
        self.ctx.set_graph_geometry(self.primitive)

    @classmethod
    def from_file(cls, scene, path, **kw):
        """The integrator over a graph file (`pbrt --graph`): load_uniform(path) or
        load_index(path) by the file's kind, as GraphIntegrator::Initialize decides, then the
        constructor's keywords."""
        if graph_io.read_kind(path) == "uniform":
            return cls(scene, load_uniform(path), **kw)
        return cls(scene, load_index(path), **kw)

    def _render_range(self, spp_begin, spp_end):
        if isinstance(self.index, capi.GraphUniform):
            self.ctx.graph_render_uniform(self.index, spp_begin, spp_end, self.seed, self.graph_from_render,
                                          view=1 if self.voxel_view else 0, light_scale=self.light_scale)
        else:
            self.ctx.graph_render(self.index, spp_begin, spp_end, self.seed, self.graph_from_render)

    def last_pass(self, max_samples=None):
        """The last pass per sample: dict of first sample index, sample count, L, lambda, pdf
        (n, 4), camera ray o, d, scatter point p (n, 3, render space) and the vertices
        averaged (count, -1 without a scatter); n = pixels x samples of that pass, element
        s * pixels + pixel. With a uniform graph count is 1 (the point's voxel has a vertex), 0
        or -1; with voxel_view p is the lit voxel's chord middle in graph space and count 1 / 0
        where a lit voxel was hit, -1 elsewhere."""
        f = self.scene.film
        npix = f.npix    # the film's pixel bounds
        ms = self.spp if max_samples is None else int(max_samples)
        first, ns, L, lam, pdf = self.ctx.last_pass_samples(npix, ms)
        o, d, p, count = self.ctx.graph_last_pass(npix, ms)
        n = npix * ns
        return dict(first=first, samples=ns, L=L, lam=lam, pdf=pdf, o=o[:n], d=d[:n], p=p[:n], count=count[:n])


# ---------------------------------------------------------------------------
# The analyzer (graph/analysis/integration_analyzer.cpp)

class GraphAnalysis:
    """IntegrationAnalyzer's counters for every pixel: (H, W) maps of the scatters analysed
    (total), those with a vertex within the vertex radius (node), those with a vertex within
    its own search range (search), the vertices in range (in_range) and the sum of their
    distances (range_sum, fp64)."""

    def __init__(self, width, height, maxdepth, spp, total, node, search, in_range, range_sum):
        self.width, self.height, self.maxdepth, self.spp = int(width), int(height), int(maxdepth), int(spp)
        shape = (self.height, self.width)
        self.total, self.node, self.search, self.in_range = (np.asarray(a, np.uint64).reshape(shape)
                                                             for a in (total, node, search, in_range))
        self.range_sum = np.asarray(range_sum, np.float64).reshape(shape)

    @staticmethod
    def _figures(total, node, search, in_range, range_sum):
        # the reference prints float ratios (0 / 0 is its NaN) and Averager::GetAverage (0 when empty)
        with np.errstate(all="ignore"):
            return dict(total=int(total), node=int(node), search=int(search), in_range=int(in_range),
                        node_ratio=float(f32(node) / f32(total)), search_ratio=float(f32(search) / f32(total)),
                        mean_range=float(f32(range_sum / in_range)) if in_range else 0.0)

    def pixel(self, x, y):
        """The reference's figures for pixel (x, y) over the samples analysed: nodeScatters,
        searchScatters, totalScatters, their ratios and rangeAverager.GetAverage()."""
        return self._figures(self.total[y, x], self.node[y, x], self.search[y, x], self.in_range[y, x],
                             self.range_sum[y, x])

    def summary(self):
        """pixel()'s figures over the whole frame (range_sum added in row-major pixel order)."""
        return self._figures(self.total.sum(), self.node.sum(), self.search.sum(), self.in_range.sum(),
                             float(np.add.reduce(self.range_sum.ravel())))

    @staticmethod
    def _line(where, f):
        return (f"{where}, {f['node']} / {f['total']} ({f['node_ratio']:g}) | {f['search']} / {f['total']} "
                f"({f['search_ratio']:g}), {f['mean_range']:g}")

    def format_line(self, x, y):
        """IntegrationAnalyzer::Render's line for one pixel (integration_analyzer.cpp:40-44)."""
        return self._line(f"[ {int(x)}, {int(y)} ]", self.pixel(x, y))

    def format_summary(self):
        return self._line("frame", self.summary())

    def ratio_maps(self):
        """(node ratio, search ratio, mean range) as float32 (H, W) images; 0 where a pixel
        analysed no scatter (or found no vertex in range)."""
        with np.errstate(all="ignore"):
            t = self.total.astype(np.float64)
            nr = np.where(self.total > 0, self.node / t, 0.0)
            sr = np.where(self.total > 0, self.search / t, 0.0)
            mr = np.where(self.in_range > 0, self.range_sum / self.in_range.astype(np.float64), 0.0)
        return nr.astype(f32), sr.astype(f32), mr.astype(f32)


class IntegrationAnalyzer:
    """IntegrationAnalyzer (graph/analysis/integration_analyzer.cpp), the fork's "analyzer"
    integrator: it follows the camera paths through the medium for up to `maxdepth` real
    scatters and asks at each whether a graph vertex lies within the vertex radius and whether
    any lies within its own render search range, and how far those are (k_graph_analyze,
    avr_graph_analyze): how well a graph serves this camera. The reference prints the figures
    for a hard-coded pixel list; here every pixel is analysed. `graph_index`, `graph_from_render`,
    `primitive` and the scene's limits are GraphIntegrator's, except that no light is needed.
    Nothing is rendered: the film is not touched."""

    def __init__(self, scene, graph_index, maxdepth=1, spp=1, seed=0, graph_from_render=None, device=0, max_paths=0,
                 primitive="box"):
        if int(maxdepth) < 0:
            raise ValueError("maxdepth must not be negative")
        self.primitive = _check_primitive(primitive)
        self.scene = scene
        self.index = graph_index
        self.maxdepth = int(maxdepth)
        self.spp = int(spp)
        self.seed = int(seed)
        self.device = int(device)
        self.graph_from_render = None if graph_from_render is None else np.asarray(graph_from_render, f32).reshape(4, 4)
        self.ctx = capi.Context(device, max_paths)
        self.ctx.set_scene(scene)
        self.ctx.set_graph_geometry(self.primitive)

    @classmethod
    def from_file(cls, scene, path, **kw):
        """The analyzer over a graph file (`pbrt --graph`): load_index(path), then the
        constructor's keywords."""
        return cls(scene, load_index(path), **kw)

    @staticmethod
    def create_params(name, params, maxdepth_override=None):
        """Constructor arguments of IntegrationAnalyzer::Create (integration_analyzer.cpp:165-174):
        "maxdepth" from the scene file (default 1), replaced by the --maxdepth option whenever
        it is given (a std::optional: 0 counts), as the fork's volpathcustom does; pixelsamples
        and seed are the sampler's."""
        if name != "analyzer":
            raise ValueError(f"{name}: integrator type unknown.")
        maxdepth = int(params.get("maxdepth", 1))
        if maxdepth_override is not None:
            maxdepth = int(maxdepth_override)
        return dict(maxdepth=maxdepth, spp=int(params.get("pixelsamples", 16)), seed=int(params.get("seed", 0)))

    @classmethod
    def create(cls, name, params, scene, graph_index=None, device=0, maxdepth_override=None, **kw):
        """Integrator::Create-style factory (cpu/integrators.cpp:3695-3700, name "analyzer")."""
        return cls(scene, graph_index, device=device, **cls.create_params(name, params, maxdepth_override), **kw)

    def analyze(self, spp_begin=0, spp_end=None, clear=True, detail=False):
        """Analyse sample indices [spp_begin, spp_end) of every pixel; returns the GraphAnalysis
        of everything analysed since the last clear. detail=True keeps the last pass's
        scatters for last_pass()."""
        if spp_end is None:
            spp_end = self.spp
        if clear:
            self.ctx.graph_analysis_clear()
        self.ctx.graph_analyze(self.index, spp_begin, spp_end, self.seed, self.maxdepth, self.graph_from_render,
                               detail=detail)
        return self.result()

    def result(self):
        f = self.scene.film
        # (the maps cover the film's pixel bounds: pixel (x, y) of a map is (x0 + x, y0 + y) of the film)
        return GraphAnalysis(f.crop_width, f.crop_height, self.maxdepth, self.spp, *self.ctx.graph_analysis_read(f.npix))

    def last_pass(self, max_samples=None):
        """The last pass of analyze(detail=True) per sample: dict of first sample index, sample
        count, camera ray o, d (n, 3), scatters analysed (count, n) and per sample `maxdepth`
        entries of the scatter point p (n, maxdepth, 3, render space), node, in_range and
        range_sum (n, maxdepth; zero past count); n = pixels x samples of that pass, element
        s * pixels + pixel."""
        f = self.scene.film
        npix = f.npix    # the film's pixel bounds
        ms = self.spp if max_samples is None else int(max_samples)
        o, d, count, p, node, in_range, range_sum = self.ctx.graph_analyze_last_pass(npix, ms, self.maxdepth)
        first, ns, _, lam, _ = self.ctx.last_pass_samples(npix, ms)
        n = npix * ns
        return dict(first=first, samples=ns, lam=lam, o=o[:n], d=d[:n], count=count[:n], p=p[:n], node=node[:n],
                    in_range=in_range[:n], range_sum=range_sum[:n])

    def stats(self):
        return self.ctx.stats()

    def close(self):
        self.ctx.close()
