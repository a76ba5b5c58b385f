"""Sequential restatement of the reference assembler, the oracle of the asm tests.

A literal transliteration of assembler/graph_wrapper.hpp and
assembler/assembler.hpp into plain Python: dictionaries for the two k-mer maps,
lists for the adjacency lists (out-edge order = creation order, as boost's vecS
keeps it), one edge record per add_edge. It shares no code with the library.
The reference itself is compiled next to this suite (oracle/ref_asm_driver.cpp,
over a stand-in for Boost.Graph) and tests/test_asm_ref_pins.py holds this file
to it, live and through tests/golden/asm_golden.npz.

Two things differ from the reference here, on purpose:
  * the sort of get_haplotypes is stable (equal scores keep discovery order).
    The reference's std::sort is not: among equal scores its order, and at the
    cut of 128 its choice, are what the C++ library's introsort makes of the
    comparison results. The library follows the reference there
    (csrc/asm_paths.cpp) and is pinned to the fixture exactly; this file is
    compared with the reference up to the order within runs of equal score
    bits, and up to which members of such a run stay where it straddles the cut;
  * more than MAX_PATHS paths in an attempt end the region as TOO_COMPLEX
    (the reference enumerates without bound).
"""
from __future__ import annotations

import math
import sys

INITIAL_KMER_SIZE = 25
KMER_SIZE_ITERATION_INCREASE = 10
MAX_KMER_ITERATIONS_TO_ATTEMPT = 9
MAX_UNIQUE_KMERS_COUNT_TO_DISCARD = 2000
DEFAULT_NUM_PATHS = 128
MIN_BASE_QUALITY_TO_USE = 10 + 33
PRUNE_FACTOR = 2
MAX_PATHS = 65536

# attempt codes and region status, the values of include/hc_asm.h
NOT_TRIED, SHORT_REF, TOO_MANY_KMERS, CYCLE, ACCEPTED = 0, 1, 2, 3, 4
OK, NO_HAPLOTYPES, TOO_COMPLEX = 0, 1, 2


class TooComplex(Exception):
    pass


class Edge:
    __slots__ = ("u", "v", "count", "is_ref", "is_on_path", "score", "seq")

    def __init__(self, u, v, seq):
        self.u, self.v, self.seq = u, v, seq
        self.count = 0
        self.is_ref = False
        self.is_on_path = False
        self.score = -sys.float_info.max


class GraphWrapper:
    def __init__(self, kmer_size):
        self.kmer_size = kmer_size
        self.kmer = []        # g[v].kmer
        self.out_edges = []   # per vertex, edges in creation order
        self.in_edges = []
        self.edges = []
        self.source = 0
        self.sink = 0
        self.paths = []
        self.vertices_on_paths = set()
        self.ref = b""
        self.read_segs = []
        self.dup_kmers = set()
        self.unique_kmers = {}

    # -- graph primitives
    def create_edge(self, u, v, is_ref):
        e = Edge(u, v, len(self.edges))
        self.edges.append(e)
        self.out_edges[u].append(e)
        self.in_edges[v].append(e)
        e.count += 1
        e.is_ref = is_ref

    def create_vertex(self, kmer):
        v = len(self.kmer)
        self.kmer.append(kmer)
        self.out_edges.append([])
        self.in_edges.append([])
        if kmer not in self.dup_kmers:
            self.unique_kmers.setdefault(kmer, v)
        return v

    def get_vertex(self, kmer):
        v = self.unique_kmers.get(kmer)
        if v is not None:
            return v
        return self.create_vertex(kmer)

    def increase_counts_backwards(self, v, kmer):
        while True:   # the reference recurses; with in_degree == 1 there is one branch
            if len(kmer) == 0:
                return
            if len(self.in_edges[v]) != 1:
                return
            e = self.in_edges[v][0]
            u = e.u
            if self.kmer[u][-1] != kmer[-1]:
                return
            e.count += 1
            v, kmer = u, kmer[:-1]

    def extend_chain(self, u, kmer, is_ref):
        for e in self.out_edges[u]:
            if self.kmer[e.v][-1] == kmer[-1]:
                e.count += 1
                return e.v
        v = self.get_vertex(kmer)
        self.create_edge(u, v, is_ref)
        return v

    def add_seq(self, seq, is_ref):
        k = self.kmer_size
        v = self.get_vertex(seq[:k])
        self.increase_counts_backwards(v, seq[:k - 1])
        if is_ref:
            self.source = v
        for i in range(1, len(seq) - k + 1):
            v = self.extend_chain(v, seq[i:i + k], is_ref)
        if is_ref:
            self.sink = v

    # -- input
    @staticmethod
    def get_dup_kmers(seq, size):
        all_kmers, dup = set(), set()
        for i in range(len(seq) - size + 1):
            kmer = seq[i:i + size]
            if kmer in all_kmers:
                dup.add(kmer)
            all_kmers.add(kmer)
        return dup

    def set_ref(self, ref):
        self.ref = ref

    def set_read(self, seq, qual):
        def usable(base, q):
            q = q - 256 if q >= 128 else q   # QUAL is a std::string: signed char
            return base != ord("N") and q >= MIN_BASE_QUALITY_TO_USE

        start = None
        for i in range(len(seq) + 1):
            if i == len(seq) or not usable(seq[i], qual[i]):
                if start is not None and i - start >= self.kmer_size:
                    self.read_segs.append(seq[start:i])
                start = None
            elif start is None:
                start = i

    def build(self):
        self.dup_kmers |= self.get_dup_kmers(self.ref, self.kmer_size)
        for seg in self.read_segs:
            self.dup_kmers |= self.get_dup_kmers(seg, self.kmer_size)
        self.add_seq(self.ref, True)
        for seg in self.read_segs:
            self.add_seq(seg, False)

    # -- acceptance
    def edge_filter(self, e):
        return e.is_ref or e.count >= PRUNE_FACTOR or len(self.out_edges[e.u]) == 1

    def has_cycles(self):
        # depth_first_search over every vertex of the filtered graph; a back edge is a cycle
        color = [0] * len(self.kmer)
        for root in range(len(self.kmer)):
            if color[root]:
                continue
            color[root] = 1
            stack = [(root, 0)]
            while stack:
                v, i = stack.pop()
                oe = self.out_edges[v]
                while i < len(oe) and not self.edge_filter(oe[i]):
                    i += 1
                if i == len(oe):
                    color[v] = 2
                    continue
                stack.append((v, i + 1))
                w = oe[i].v
                if color[w] == 1:
                    return True
                if color[w] == 0:
                    color[w] = 1
                    stack.append((w, 0))
        return False

    def unique_kmers_count(self):
        return len(self.unique_kmers)

    # -- paths
    def path_finder(self, frm, to, path):
        path.append(frm)
        if frm == to:
            self.paths.append(list(path))
            if len(self.paths) > MAX_PATHS:
                raise TooComplex()
            self.vertices_on_paths.update(path)
        else:
            for e in self.out_edges[frm]:
                if e.is_ref or e.count >= PRUNE_FACTOR or len(self.out_edges[frm]) == 1:
                    if e.v not in path:
                        self.path_finder(e.v, to, path)
        path.pop()

    def edge(self, u, v):
        for e in self.out_edges[u]:
            if e.v == v:
                return e
        raise KeyError((u, v))

    def find_paths(self):
        old = sys.getrecursionlimit()
        sys.setrecursionlimit(max(old, 4 * len(self.kmer) + 1000))
        try:
            self.path_finder(self.source, self.sink, [])
        finally:
            sys.setrecursionlimit(old)
        for path in self.paths:
            for u, v in zip(path, path[1:]):
                self.edge(u, v).is_on_path = True
        for v in self.vertices_on_paths:
            edges = [e for e in self.out_edges[v] if e.is_on_path]
            total = 0.0
            for e in edges:
                total += e.count
            for e in edges:
                e.score = math.log10(e.count / total)
        haps = []
        for path in self.paths:
            seq = bytearray(self.kmer[path[0]])
            score = 0.0
            for u, v in zip(path, path[1:]):
                seq.append(self.kmer[v][-1])
                score += self.edge(u, v).score
            haps.append((bytes(seq), score))
        haps.sort(key=lambda h: -h[1])   # stable: this file's tie rule, not the reference's (see the docstring)
        self.sorted_haps = haps          # before the cut: what a run of equal scores at the cut is compared against
        return haps[:DEFAULT_NUM_PATHS]

    def reduced_graph(self):
        """The on-path edges in creation order: (from, to, last byte, count, is_ref, seq)."""
        return [(e.u, e.v, self.kmer[e.v][-1], e.count, int(e.is_ref), e.seq) for e in self.edges if e.is_on_path]


def assemble(reads, ref):
    """reads: [(bases, quals)] bytes; ref: bytes. Returns a dict with status,
    kmer_size, attempts (9 codes), haps [(bases, score)], n_paths, and of the
    accepted attempt the graph (reduced_graph), source, sink and the whole
    GraphWrapper under "g"."""
    attempts = [NOT_TRIED] * MAX_KMER_ITERATIONS_TO_ATTEMPT
    out = dict(status=NO_HAPLOTYPES, kmer_size=0, attempts=attempts, haps=[], n_paths=0, graph=[], source=-1,
               sink=-1, g=None)
    k = INITIAL_KMER_SIZE
    for it in range(MAX_KMER_ITERATIONS_TO_ATTEMPT):
        if len(ref) < k:
            attempts[it] = SHORT_REF
        else:
            g = GraphWrapper(k)
            g.set_ref(ref)
            for seq, qual in reads:
                g.set_read(seq, qual)
            g.build()
            if g.unique_kmers_count() > MAX_UNIQUE_KMERS_COUNT_TO_DISCARD:
                attempts[it] = TOO_MANY_KMERS
            elif g.has_cycles():
                attempts[it] = CYCLE
            else:
                attempts[it] = ACCEPTED
                out.update(kmer_size=k, g=g, source=g.source, sink=g.sink)
                try:
                    haps = g.find_paths()
                except TooComplex:
                    out.update(status=TOO_COMPLEX, n_paths=MAX_PATHS + 1)
                    return out
                out.update(haps=haps, n_paths=len(g.paths), graph=g.reduced_graph())
                if haps:
                    out["status"] = OK
                    return out
        k += KMER_SIZE_ITERATION_INCREASE
    return out
