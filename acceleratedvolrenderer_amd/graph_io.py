"""Graph files in the reference's text format (src/graph/graph.cpp:15-24 Point3 streaming,
:237-416 Graph::WriteToStream / ReadFromStream, :418-433 WriteToDisk, :566-577 and :644-655
the uniform and free headers): what graph_maker writes and `pbrt --graph` reads.

    <description>                                   one token ("basic")
    free <vertexRadius>            or               uniform <spacing>
    <useCoors> <useSamples> <useRayVertexTypes> <useLighting> <useRenderSearchRange>   True / False
    <curVertexId> <curEdgeId> <curPathId> <numVertices> <numEdges> <numPaths>
    <id> <x> <y> <z> [type] [lightScalar] [samples] [renderSearchRange] [cx cy cz]    per vertex
    <id> <from> <to> [samples]                                                      per edge
    <id> <length> <vertex id> ...                                                   per path

The four header lines have single spaces between their fields and none at the end; on
vertex, edge and path lines every field is followed by one space, the last one too, then the
newline. The reader takes whitespace-separated tokens as the reference's operator>> does, so
line breaks carry no meaning to it; vertex lines may come in any id order (the reference
writes an unordered_map) and are placed by id.

A uniform graph's file (write_uniform_graph) has useCoors True: the vertex's three integer
lattice coordinates follow its data.

Floats are written as %.{precision}g. precision 6 is the text of the reference's ostream at
its default precision; the default 9 lets every float32 survive a round trip exactly. The
reference reads either.
"""
import numpy as np

f32 = np.float32

FLAG_NAMES = ("use_coors", "use_samples", "use_ray_vertex_types", "use_lighting", "use_render_search_range")


class GraphFile:
    """What read_graph returns. Vertex arrays are indexed by vertex id; a field whose stream
    flag is False is None.

    description, kind ("free" or "uniform"), radius (free: vertexRadius) or spacing (uniform),
    flags (dict over FLAG_NAMES), cur_vertex_id, cur_edge_id, cur_path_id;
    points (n, 3) float32, vertex_type, light_scalar, samples, search_range, coors (n, 3) int32;
    file_ids: the vertex ids in the order of their lines (the reference adds vertices in that order);
    edge_id, edge_from, edge_to, edge_samples; paths: list of (id, int32 vertex ids)."""

    def __init__(self):
        self.description = "basic"
        self.kind = "free"
        self.radius = None
        self.spacing = None
        self.flags = dict.fromkeys(FLAG_NAMES, False)
        self.cur_vertex_id = self.cur_edge_id = self.cur_path_id = 0
        self.points = np.zeros((0, 3), f32)
        self.file_ids = np.zeros(0, np.int32)
        self.vertex_type = self.light_scalar = self.samples = self.search_range = self.coors = None
        self.edge_id = self.edge_from = self.edge_to = np.zeros(0, np.int32)
        self.edge_samples = None
        self.paths = []

    @property
    def num_vertices(self):
        return len(self.points)


class _Tokens:
    """The stream's whitespace-separated tokens with the line each came from (for errors)."""

    def __init__(self, path, text):
        self.path = path
        self.lines = text.split("\n")
        self.tok = text.split()
        self.pos = 0
        self._line_of = None

    def line(self, i):
        """1-based line number of token i (of the last line when i is past the end)."""
        if self._line_of is None:
            counts = np.array([len(l.split()) for l in self.lines], np.int64)
            self._line_of = np.repeat(np.arange(1, len(self.lines) + 1), counts)
        if len(self._line_of) == 0:
            return 1
        return int(self._line_of[min(i, len(self._line_of) - 1)])

    def error(self, i, what):
        if i >= len(self.tok):
            return ValueError(f"{self.path}: line {self.line(i)}: file ends where {what} is expected")
        return ValueError(f"{self.path}: line {self.line(i)}: {what} expected, found {self.tok[i]!r}")

    def take(self, n, what):
        """The next n tokens as a list."""
        if self.pos + n > len(self.tok):
            raise self.error(len(self.tok), what)
        out = self.tok[self.pos:self.pos + n]
        self.pos += n
        return out

    def word(self, what):
        return self.take(1, what)[0]

    def convert(self, cast, what):
        i = self.pos
        t = self.word(what)
        try:
            return cast(t)
        except ValueError:
            raise self.error(i, what) from None

    def table(self, rows, kinds, what):
        """rows x len(kinds) tokens as one array per column; kinds: "i" int, "f" float."""
        w = len(kinds)
        start = self.pos
        block = np.array(self.take(rows * w, what), dtype=object).reshape(rows, w) if rows else np.zeros((0, w), object)
        cols = []
        for c, kind in enumerate(kinds):
            col = block[:, c].tolist()
            try:
                if kind == "i":
                    cols.append(np.array([int(t) for t in col], np.int64))
                else:
                    cols.append(np.array([float(t) for t in col], np.float64).astype(f32))
            except (ValueError, OverflowError):
                cast = int if kind == "i" else float
                for r, t in enumerate(col):   # find the token that failed
                    try:
                        cast(t)
                    except (ValueError, OverflowError):
                        raise self.error(start + r * w + c, "an integer" if kind == "i" else "a number") from None
                raise
        return cols


def read_kind(path):
    """"free" or "uniform": the second token of a graph file, which GraphIntegrator::Initialize
    (graph_integrator.cpp:29-33) reads to choose its branch."""
    with open(path, "r") as fh:
        tk = _Tokens(path, fh.read(4096))
    tk.word("the description")
    i = tk.pos
    kind = tk.word('"free" or "uniform"')
    if kind not in ("free", "uniform"):
        raise tk.error(i, '"free" or "uniform"')
    return kind


def read_graph(path):
    """Read a graph file (Graph::ReadFromStream, graph.cpp:347-416, under the free / uniform
    header, :572-577 / :650-655) into a GraphFile. ValueError with the line number on a short
    or malformed stream, and when the vertex ids are not exactly 0..n-1 (CheckSequentialIds)."""
    with open(path, "r") as fh:
        tk = _Tokens(path, fh.read())
    g = GraphFile()
    g.description = tk.word("the description")
    i = tk.pos
    g.kind = tk.word('"free" or "uniform"')
    if g.kind not in ("free", "uniform"):
        raise tk.error(i, '"free" or "uniform"')
    size = tk.convert(float, "the vertex radius" if g.kind == "free" else "the spacing")
    if g.kind == "free":
        g.radius = f32(size)
    else:
        g.spacing = f32(size)
    for name in FLAG_NAMES:
        i = tk.pos
        t = tk.word("True or False")
        if t not in ("True", "False"):
            raise tk.error(i, "True or False")
        g.flags[name] = t == "True"
    g.cur_vertex_id = tk.convert(int, "curVertexId")
    g.cur_edge_id = tk.convert(int, "curEdgeId")
    g.cur_path_id = tk.convert(int, "curPathId")
    counts = []
    for what in ("the vertex count", "the edge count", "the path count"):
        i = tk.pos
        v = tk.convert(int, what)
        if v < 0:
            raise tk.error(i, what)
        counts.append(v)
    nv, ne, npaths = counts
    fl = g.flags
    # WriteVertexData's order: type, lighting, samples, search range; then the coors
    kinds = "ifff" + ("i" if fl["use_ray_vertex_types"] else "") + ("f" if fl["use_lighting"] else "") \
        + ("i" if fl["use_samples"] else "") + ("f" if fl["use_render_search_range"] else "") \
        + ("iii" if fl["use_coors"] else "")
    start = tk.pos
    cols = tk.table(nv, kinds, "a vertex line")
    ids = cols[0]
    order = np.argsort(ids, kind="stable")
    bad = np.nonzero(ids[order] != np.arange(nv))[0]
    if len(bad):
        b = int(bad[0])
        seen = int(ids[order][b])
        what = f"vertex id {b} is missing" if seen > b else f"vertex id {seen} is out of place or repeated"
        raise ValueError(f"{path}: line {tk.line(start + int(order[b]) * len(kinds))}: {what}: "
                         f"Graph must have sequential vertex ids 0..{nv - 1}")
    g.file_ids = ids.astype(np.int32)
    cols = [c[order] for c in cols]
    g.points = np.stack(cols[1:4], axis=1).astype(f32) if nv else np.zeros((0, 3), f32)
    c = 4
    if fl["use_ray_vertex_types"]:
        g.vertex_type = cols[c].astype(np.int32)
        c += 1
    if fl["use_lighting"]:
        g.light_scalar = cols[c]
        c += 1
    if fl["use_samples"]:
        g.samples = cols[c].astype(np.int32)
        c += 1
    if fl["use_render_search_range"]:
        g.search_range = cols[c]
        c += 1
    if fl["use_coors"]:
        g.coors = np.stack(cols[c:c + 3], axis=1).astype(np.int32) if nv else np.zeros((0, 3), np.int32)
    ecols = tk.table(ne, "iii" + ("i" if fl["use_samples"] else ""), "an edge line")
    g.edge_id, g.edge_from, g.edge_to = (e.astype(np.int32) for e in ecols[:3])
    if fl["use_samples"]:
        g.edge_samples = ecols[3].astype(np.int32)
    for _ in range(npaths):
        pid = tk.convert(int, "a path id")
        i = tk.pos
        length = tk.convert(int, "a path length")
        if length < 0:
            raise tk.error(i, "a path length")
        g.paths.append((pid, tk.table(length, "i", "a path's vertex ids")[0].astype(np.int32)))
    return g


def write_graph(path, graph, light_scalar=None, description="basic", precision=9, edges=False):
    """Write `graph` (a graph.FreeGraph, a GraphFile, or anything with points, radius and
    optionally search_range, edge_from / edge_to / edge_samples) as FreeGraph::WriteToStream
    does (graph.cpp:644-648, :284-345), with graph_maker's stream flags (graph_maker.cpp:
    171-173): vertices only, useLighting with `light_scalar` (default: the graph's own
    light_scalar), useRenderSearchRange when the graph has search ranges. edges=True also
    writes the edges and sets useSamples, which puts the samples on vertex and edge lines.
    curPathId is written as 0: path information is not kept here."""
    pts = np.ascontiguousarray(graph.points, f32).reshape(-1, 3)
    n = len(pts)
    if light_scalar is None:
        light_scalar = getattr(graph, "light_scalar", None)
    rng = getattr(graph, "search_range", None)
    smp = getattr(graph, "samples", None) if edges else None
    if edges and smp is None:
        raise ValueError("write_graph: edges=True needs the vertices' samples")
    for name, a in (("light_scalar", light_scalar), ("search_range", rng), ("samples", smp)):
        if a is not None and len(a) != n:
            raise ValueError(f"write_graph: one {name} per vertex")
    if not isinstance(description, str) or len(description.split()) != 1:
        raise ValueError("write_graph: the description is one token without whitespace")
    p = int(precision)
    if p < 1:
        raise ValueError("write_graph: precision must be positive")
    ff = f"%.{p}g "
    nedges = len(graph.edge_from) if getattr(graph, "edge_from", None) is not None else 0
    flags = (False, bool(edges), False, light_scalar is not None, rng is not None)
    fmt = "%d " + ff * 3 + (ff if flags[3] else "") + ("%d " if flags[1] else "") + (ff if flags[4] else "") + "\n"
    cols = [range(n)] + [pts[:, a].astype(np.float64).tolist() for a in range(3)]
    if flags[3]:
        cols.append(np.asarray(light_scalar, f32).astype(np.float64).tolist())
    if flags[1]:
        cols.append(np.asarray(smp, np.int64).tolist())
    if flags[4]:
        cols.append(np.asarray(rng, f32).astype(np.float64).tolist())
    with open(path, "w", newline="\n") as fh:
        fh.write(f"{description}\n")
        fh.write("free %.*g\n" % (p, float(f32(graph.radius))))
        fh.write(" ".join("True" if f else "False" for f in flags) + "\n")
        fh.write(f"{n} {nedges} 0 {n} {nedges if edges else 0} 0\n")
        fh.writelines(fmt % row for row in zip(*cols))
        if edges:
            es = np.asarray(graph.edge_samples, np.int64).tolist()
            fh.writelines("%d %d %d %d \n" % row for row in zip(range(nedges), np.asarray(graph.edge_from).tolist(),
                                                               np.asarray(graph.edge_to).tolist(), es))


def write_uniform_graph(path, uniform, description="basic", precision=9):
    """Write a uniform graph (a capi.GraphUniform, a graph.UniformGraph, or anything with coors
    (m, 3), light_scalar and spacing) as UniformGraph::WriteToStream does (graph.cpp:566-570,
    :284-345): "uniform <spacing>", vertices only, useLighting, and useCoors True with the three
    lattice coordinates after the vertex data (:314-315). The point of a vertex is
    (float)coors * spacing (:555). precision as write_graph's."""
    coors = np.ascontiguousarray(uniform.coors, np.int32).reshape(-1, 3)
    light = np.ascontiguousarray(uniform.light_scalar, f32).reshape(-1)
    n = len(coors)
    if len(light) != n:
        raise ValueError("write_uniform_graph: one light_scalar per vertex")
    if not isinstance(description, str) or len(description.split()) != 1:
        raise ValueError("write_uniform_graph: the description is one token without whitespace")
    p = int(precision)
    if p < 1:
        raise ValueError("write_uniform_graph: precision must be positive")
    spacing = f32(uniform.spacing)
    pts = (coors.astype(f32) * spacing).astype(f32)
    ff = f"%.{p}g "
    fmt = "%d " + ff * 4 + "%d %d %d \n"
    cols = [range(n)] + [pts[:, a].astype(np.float64).tolist() for a in range(3)] + [light.astype(np.float64).tolist()] \
        + [coors[:, a].tolist() for a in range(3)]
    with open(path, "w", newline="\n") as fh:
        fh.write(f"{description}\n")
        fh.write("uniform %.*g\n" % (p, float(spacing)))
        fh.write("True False False True False\n")
        fh.write(f"{n} 0 0 {n} 0 0\n")
        fh.writelines(fmt % row for row in zip(*cols))
