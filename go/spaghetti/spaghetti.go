// Package spaghetti is the cgo binding of libspaghetti_rank.so (include/spaghetti_rank.h).
//
// It is the ONLY file that touches C.  go/ranking and go/retrieval keep the reference's
// exported signatures (ranking/pagerank.go:14, ranking/term_weighting.go:10,
// retrieval/main_retrieve.go:15) and call into this package.
//
// NOTE: written against the header but NOT compiled in the build image (no Go toolchain
// there, SURVEY.md §8c); the same entry points are exercised through Python ctypes
// (spaghettisearch_amd/_lib.py) by the test-suite.
//
// Error policy: every non-zero status becomes panic(err), like the reference
// (pagerank.go:20,29,49,57,76,81; term_weighting.go:14,23,34,48,52).
package spaghetti

/*
#cgo CFLAGS: -I${SRCDIR}/../../include
#cgo LDFLAGS: -L${SRCDIR}/../../spaghettisearch_amd -lspaghetti_rank -Wl,-rpath,${SRCDIR}/../../spaghettisearch_amd
#include <stdlib.h>
#include "spaghetti_rank.h"
*/
import "C"

import (
	"fmt"
	"math"
	"os"
	"runtime"
	"strconv"
	"sync"
	"time"
	"unsafe"
)

// Per-request limits of the scorer (a batch that breaks one is refused as a whole: callers validate first).
const (
	MaxQueryTerms  = int(C.SS_MAX_QUERY_TERMS)
	MaxPhraseTerms = int(C.SS_MAX_PHRASE_TERMS)
)

// Hit mirrors ss_hit.
type Hit struct {
	Doc      uint32
	Title    float64
	Body     float64
	PageRank float64
	Final    float64
}

type Ctx struct{ h *C.ss_ctx }
type Graph struct {
	h   *C.ss_graph
	ctx *Ctx
	N   uint64
}
type Index struct {
	h      *C.ss_index
	ctx    *Ctx
	NDocs  uint64
	NTerms uint64
	NPost  uint64
}
type Scorer struct {
	h         *C.ss_scorer
	ctx       *Ctx
	nDocs     uint64 // the title table's doc count when the scorer was created: sizes DocFieldMasks' words
	nFields   int    // fields registered by SetDocFields: sizes HitFields' values
	nMasks    int    // allow-lists registered by SetDocMasks: sizes FacetCounts' mask counts
	vecDim    int    // dim of the table registered by SetDocVectors: sizes the query vectors
	nVecLists int    // lists registered by SetVectorLists: sizes the probes of VectorTopKProbed
}

var (
	once   sync.Once
	global *Ctx
)

// statusErr turns a library status into an error (nil for SS_OK).
func statusErr(c *Ctx, rc C.int32_t, what string) error {
	if rc == C.SS_OK {
		return nil
	}
	var h *C.ss_ctx
	if c != nil {
		h = c.h
	}
	return fmt.Errorf("%s: status %d: %s", what, int(rc), C.GoString(C.ss_last_error(h)))
}

func check(c *Ctx, rc C.int32_t, what string) {
	if err := statusErr(c, rc, what); err != nil {
		panic(err)
	}
}

// JobInfo is this process's place in a multi-GPU job (SS_RANK / SS_WORLD; absent = a job of one).
type JobInfo struct{ Rank, World int }

func Job() JobInfo {
	w, _ := strconv.Atoi(os.Getenv("SS_WORLD"))
	r, _ := strconv.Atoi(os.Getenv("SS_RANK"))
	if w < 2 {
		return JobInfo{0, 1}
	}
	return JobInfo{r, w}
}

// Default returns the process-wide context (one process per GPU; the launcher pins the GPU with HIP_VISIBLE_DEVICES, so the
// device index is 0).  In a multi-GPU job it also joins the job's RCCL communicator through SS_COMM_ID_FILE:
//   - the file holds the 128-byte id followed by the job's nonce SS_JOB_ID (the launcher gives every start of the job a
//     fresh value, e.g. its pid + start time); a reader accepts the file only when the nonce is its own, so a file left
//     behind by an earlier or crashed job is never used;
//   - rank 0 removes whatever is at the path first, writes temp file + rename, and removes the file again once
//     CommInit has returned (ncclCommInitRank is collective: every rank holds the id by then);
//   - the other ranks wait SS_COMM_TIMEOUT_S seconds at most (default 120) and then panic, so that a job whose rank 0
//     never came up exits non-zero instead of hanging.
func Default() *Ctx {
	once.Do(func() {
		// the header this package was compiled against and the library that got loaded must be the same ABI (4: submit / collect,
		// late-completing ss_graph_create)
		if v := int(C.ss_abi_version()); v != int(C.SS_ABI_VERSION) {
			panic(fmt.Errorf("libspaghetti_rank: ABI version %d, this package was built against %d", v, int(C.SS_ABI_VERSION)))
		}
		var h *C.ss_ctx
		check(nil, C.ss_init(0, &h), "ss_init")
		global = &Ctx{h}
		if job := Job(); job.World > 1 {
			path := os.Getenv("SS_COMM_ID_FILE")
			if path == "" {
				panic(fmt.Errorf("SS_WORLD=%d needs SS_COMM_ID_FILE", job.World))
			}
			nonce := []byte(os.Getenv("SS_JOB_ID"))
			if len(nonce) == 0 {
				panic(fmt.Errorf("SS_WORLD=%d needs SS_JOB_ID (a value unique to this start of the job)", job.World))
			}
			var id []byte
			if job.Rank == 0 {
				_ = os.Remove(path)
				id = CommUniqueID()
				if err := os.WriteFile(path+".tmp", append(append([]byte{}, id...), nonce...), 0o600); err != nil {
					panic(err)
				}
				if err := os.Rename(path+".tmp", path); err != nil {
					panic(err)
				}
			} else {
				limit := 120
				if v, err := strconv.Atoi(os.Getenv("SS_COMM_TIMEOUT_S")); err == nil && v > 0 {
					limit = v
				}
				deadline := time.Now().Add(time.Duration(limit) * time.Second)
				for id == nil {
					b, err := os.ReadFile(path)
					if err == nil && len(b) == C.SS_COMM_ID_BYTES+len(nonce) && string(b[C.SS_COMM_ID_BYTES:]) == string(nonce) {
						id = b[:C.SS_COMM_ID_BYTES]
						break
					}
					if time.Now().After(deadline) {
						panic(fmt.Errorf("rank %d: no communicator id for job %q in %s after %d s", job.Rank, string(nonce), path, limit))
					}
					time.Sleep(50 * time.Millisecond)
				}
			}
			global.CommInit(id, job.Rank, job.World)
			if job.Rank == 0 {
				_ = os.Remove(path)
			}
		}
	})
	return global
}

// OptionDefault restores an option's default (SS_OPTION_DEFAULT).
const OptionDefault = int64(math.MinInt64)

// SetOption sets a named tuning option of the context (ss_set_option; the names are listed in the header).
func (c *Ctx) SetOption(name string, value int64) {
	cs := C.CString(name)
	defer C.free(unsafe.Pointer(cs))
	check(c, C.ss_set_option(c.h, cs, C.int64_t(value)), "ss_set_option")
}

// CommSplit replaces the context's communicator by the sub-communicator of the ranks that pass the same color (2-D
// decomposition: topic groups x doc shards).
func (c *Ctx) CommSplit(color, key int) {
	check(c, C.ss_comm_split(c.h, C.int32_t(color), C.int32_t(key)), "ss_comm_split")
}

func u64p(s []uint64) *C.uint64_t {
	if len(s) == 0 {
		return nil
	}
	return (*C.uint64_t)(unsafe.Pointer(&s[0]))
}
func u32p(s []uint32) *C.uint32_t {
	if len(s) == 0 {
		return nil
	}
	return (*C.uint32_t)(unsafe.Pointer(&s[0]))
}
func i32p(s []int32) *C.int32_t {
	if len(s) == 0 {
		return nil
	}
	return (*C.int32_t)(unsafe.Pointer(&s[0]))
}
func f32p(s []float32) *C.float {
	if len(s) == 0 {
		return nil
	}
	return (*C.float)(unsafe.Pointer(&s[0]))
}
func f64p(s []float64) *C.double {
	if len(s) == 0 {
		return nil
	}
	return (*C.double)(unsafe.Pointer(&s[0]))
}

// NewGraph uploads the out-edge CSR of forw[2] (parent -> children).  The library copies the
// slices before returning (cgo pointer rules), so they may be garbage collected afterwards.
func (c *Ctx) NewGraph(outPtr []uint64, outDst []uint32) *Graph {
	n := uint64(len(outPtr) - 1)
	var h *C.ss_graph
	check(c, C.ss_graph_create(c.h, C.uint64_t(n), C.uint64_t(len(outDst)), u64p(outPtr), u32p(outDst), 0, 1, &h), "ss_graph_create")
	return &Graph{h, c, n}
}
func (g *Graph) Close() { C.ss_graph_destroy(g.h) }

// ApplyDelta patches the resident link graph: the out-edges of changed[i] become newChildren[newPtr[i]:newPtr[i+1]],
// nNodesNew >= N admits new pages (ss_graph_apply_delta; indexer.go:301-304 rewrites forw[2] of a re-crawled page).
func (g *Graph) ApplyDelta(nNodesNew uint64, changed []uint32, newPtr []uint64, newChildren []uint32) {
	check(g.ctx, C.ss_graph_apply_delta(g.h, C.uint64_t(nNodesNew), C.uint64_t(len(changed)), u32p(changed), u64p(newPtr), u32p(newChildren)),
		"ss_graph_apply_delta")
	g.N = nNodesNew
}

// Directions of TopLinks / HitLinks.
const (
	LinksParents  = int(C.SS_LINKS_PARENTS)
	LinksChildren = int(C.SS_LINKS_CHILDREN)
	MaxLinks      = int(C.SS_MAX_LINKS)
)

// SetLinkKey registers the per-node key that orders TopLinks / HitLinks (one value per node, say one topic's PageRank row;
// copied); nil clears it.  A successful ApplyDelta clears it too.
func (g *Graph) SetLinkKey(key []float64) {
	check(g.ctx, C.ss_graph_set_link_key(g.h, f64p(key)), "ss_graph_set_link_key")
}

// Links is one row of TopLinks / HitLinks: the best distinct parents or children of a node (key descending, then id; NaN last;
// ascending id without a key) and the number of edges of the row, duplicates counted.
type Links struct {
	Nodes  []uint32
	Degree uint32
}

func linkRows(rows, m int, links []uint32, nOut []int32, degree []uint32, written func(int) bool) []Links {
	out := make([]Links, rows)
	for r := 0; r < rows; r++ {
		if written(r) {
			out[r] = Links{append([]uint32(nil), links[r*m:r*m+int(nOut[r])]...), degree[r]}
		}
	}
	return out
}

// TopLinks is ss_graph_top_links: what Rank_combined.Parents / .Children (retrieval/util.go:25-36) carry, as node ids.  A node id
// the graph does not hold gives an empty row.
func (g *Graph) TopLinks(dir int, nodes []uint32, m int) ([]Links, error) {
	n := len(nodes)
	if n == 0 {
		return nil, nil
	}
	links := make([]uint32, n*m)
	nOut := make([]int32, n)
	degree := make([]uint32, n)
	rc := C.ss_graph_top_links(g.h, C.int32_t(dir), C.uint64_t(n), u32p(nodes), C.int32_t(m), u32p(links), i32p(nOut), u32p(degree))
	if err := statusErr(g.ctx, rc, "ss_graph_top_links"); err != nil {
		return nil, err
	}
	return linkRows(n, m, links, nOut, degree, func(int) bool { return true }), nil
}

// HitLinks is ss_graph_hit_links: out[q][j] describes hits[q][j].Doc taken as a node id.  Only the hits' Doc is read.
func (g *Graph) HitLinks(dir int, hits [][]Hit, m int) ([][]Links, error) {
	nq := len(hits)
	if nq == 0 {
		return nil, nil
	}
	k := 1
	for q := 0; q < nq; q++ {
		if len(hits[q]) > k {
			k = len(hits[q])
		}
	}
	raw := make([]C.ss_hit, nq*k)
	nHits := make([]int32, nq)
	for q := 0; q < nq; q++ {
		nHits[q] = int32(len(hits[q]))
		for j, h := range hits[q] {
			raw[q*k+j].doc = C.uint32_t(h.Doc)
		}
	}
	links := make([]uint32, nq*k*m)
	nOut := make([]int32, nq*k)
	degree := make([]uint32, nq*k)
	rc := C.ss_graph_hit_links(g.h, C.int32_t(dir), C.int32_t(nq), C.int32_t(k), (*C.ss_hit)(unsafe.Pointer(&raw[0])), i32p(nHits),
		C.int32_t(m), u32p(links), i32p(nOut), u32p(degree))
	if err := statusErr(g.ctx, rc, "ss_graph_hit_links"); err != nil {
		return nil, err
	}
	flat := linkRows(nq*k, m, links, nOut, degree, func(r int) bool { return r%k < int(nHits[r/k]) })
	out := make([][]Links, nq)
	for q := 0; q < nq; q++ {
		out[q] = flat[q*k : q*k+len(hits[q])]
	}
	return out, nil
}

// PageRankTeleport is the opt-in topic-sensitive run (SURVEY.md §8f-3): sets[k] = DISTINCT node ids of topic k's
// teleport set (empty = the reference's uniform teleport for that topic).  rank[k*N+v], iters[k].
func (g *Graph) PageRankTeleport(d, eps float64, nTopic []int32, sets [][]uint32) ([]float64, []int32) {
	k := len(nTopic)
	var pr *C.ss_pr
	check(g.ctx, C.ss_pr_create(g.h, C.double(d), C.double(eps), 0, C.int32_t(k), i32p(nTopic), &pr), "ss_pr_create")
	defer C.ss_pr_destroy(pr)
	setPtr := make([]uint64, k+1)
	var nodes []uint32
	for i, s := range sets {
		nodes = append(nodes, s...)
		setPtr[i+1] = uint64(len(nodes))
	}
	check(g.ctx, C.ss_pr_set_teleport(pr, u64p(setPtr), u32p(nodes)), "ss_pr_set_teleport")
	check(g.ctx, C.ss_pr_begin(pr), "ss_pr_begin")
	iters := make([]int32, k)
	var nActive, sweeps C.int32_t = C.int32_t(k), 0
	for nActive > 0 {
		check(g.ctx, C.ss_pr_step(pr, 8), "ss_pr_step")
		check(g.ctx, C.ss_pr_status(pr, i32p(iters), &nActive, &sweeps, nil, nil), "ss_pr_status")
	}
	rank := make([]float64, uint64(k)*g.N)
	check(g.ctx, C.ss_pr_read(pr, f64p(rank)), "ss_pr_read")
	return rank, iters
}

// ---- several GPUs: one process (= one context) per GPU, collectives inside the library (RCCL over xGMI) ----
//
// SS_RANK / SS_WORLD / SS_COMM_ID_FILE in the environment describe the job (a launcher starts one crawl process per
// GPU with SS_RANK = 0..SS_WORLD-1 and HIP_VISIBLE_DEVICES set to its GPU).  Rank 0 writes the 128-byte communicator
// id to SS_COMM_ID_FILE, the others wait for the file.  Without SS_WORLD the process is the whole job (world 1).

// CommInit joins this context to the job's communicator.  Blocks until every rank has joined.
func (c *Ctx) CommInit(id []byte, rank, world int) {
	if len(id) != C.SS_COMM_ID_BYTES {
		panic(fmt.Errorf("communicator id must be %d bytes", int(C.SS_COMM_ID_BYTES)))
	}
	check(c, C.ss_comm_init(c.h, unsafe.Pointer(&id[0]), C.int32_t(rank), C.int32_t(world)), "ss_comm_init")
}

// CommUniqueID is called by rank 0 only.
func CommUniqueID() []byte {
	id := make([]byte, C.SS_COMM_ID_BYTES)
	check(nil, C.ss_comm_unique_id(unsafe.Pointer(&id[0])), "ss_comm_unique_id")
	return id
}

// AllReduceU64 sums buf over the ranks in place (whole-corpus document frequencies of a doc-range-sharded index).
func (c *Ctx) AllReduceU64(buf []uint64) {
	check(c, C.ss_comm_allreduce_u64(c.h, u64p(buf), C.uint64_t(len(buf))), "ss_comm_allreduce_u64")
}

// NewGraphShard uploads the WHOLE out-edge CSR and keeps the destination rows of shard `rank` of `world`.
func (c *Ctx) NewGraphShard(outPtr []uint64, outDst []uint32, rank, world int) *Graph {
	n := uint64(len(outPtr) - 1)
	var h *C.ss_graph
	check(c, C.ss_graph_create(c.h, C.uint64_t(n), C.uint64_t(len(outDst)), u64p(outPtr), u32p(outDst), C.int32_t(rank), C.int32_t(world), &h),
		"ss_graph_create")
	return &Graph{h, c, n}
}

// PageRankSharded runs this rank's part of the doc-range-sharded power iteration (one RCCL all-gather per sweep inside
// the library): ids[r] = node id of local row r, rank[k*rows+r], iters[k].  Every process writes its own rows of forw[3].
func (g *Graph) PageRankSharded(d, eps float64, nTopic []int32) ([]uint32, []float64, []int32) {
	var info C.ss_graph_info
	check(g.ctx, C.ss_graph_get_info(g.h, &info), "ss_graph_get_info")
	rows := uint64(info.n_rows_local)
	k := len(nTopic)
	ids := make([]uint32, rows)
	rank := make([]float64, uint64(k)*rows)
	iters := make([]int32, k)
	check(g.ctx, C.ss_pagerank_run_sharded(g.h, C.double(d), C.double(eps), 0, C.int32_t(k), i32p(nTopic), 0, u32p(ids), f64p(rank), i32p(iters)),
		"ss_pagerank_run_sharded")
	return ids, rank, iters
}

// PageRank runs all topics to convergence: rank[k*N+v], iters[k].
func (g *Graph) PageRank(d, eps float64, nTopic []int32) ([]float64, []int32) {
	k := len(nTopic)
	rank := make([]float64, uint64(k)*g.N)
	iters := make([]int32, k)
	check(g.ctx, C.ss_pagerank_run(g.h, C.double(d), C.double(eps), 0, C.int32_t(k), i32p(nTopic), f64p(rank), i32p(iters)), "ss_pagerank_run")
	return rank, iters
}

func (c *Ctx) NewIndex(nDocs uint64, termPtr []uint64, postDoc []uint32, postTf []float32) *Index {
	var h *C.ss_index
	nT := uint64(len(termPtr) - 1)
	check(c, C.ss_index_create(c.h, C.uint64_t(nDocs), C.uint64_t(nT), u64p(termPtr), u32p(postDoc), f32p(postTf), &h), "ss_index_create")
	return &Index{h, c, nDocs, nT, uint64(len(postDoc))}
}
func (ix *Index) Close() { check(ix.ctx, C.ss_index_destroy(ix.h), "ss_index_destroy") }

// TfIdfBuild = ranking.UpdateTermWeights' arithmetic; returns the new weights and magnitudes.
func (ix *Index) TfIdfBuild(totalDocs uint64) (w []float32, mag []float64) {
	w = make([]float32, ix.NPost)
	mag = make([]float64, ix.NDocs)
	check(ix.ctx, C.ss_tfidf_build(ix.h, C.uint64_t(totalDocs), f32p(w), f64p(mag), nil), "ss_tfidf_build")
	return
}
func (ix *Index) SetPositions(posPtr []uint64, pos []float32) {
	check(ix.ctx, C.ss_index_set_positions(ix.h, u64p(posPtr), f32p(pos)), "ss_index_set_positions")
}

// SetDocFreq: multi-GPU doc-range shards only — df[t] = length of term t's whole posting list
// (term_weighting.go:37 len(docs)), summed over the shards by the caller.  Call before TfIdfBuild.
func (ix *Index) SetDocFreq(df []uint64) {
	check(ix.ctx, C.ss_index_set_doc_freq(ix.h, u64p(df)), "ss_index_set_doc_freq")
}

// Delta is what indexer.checkAndUpdate (indexer/indexer.go:420-641) and the re-index after it change in ONE inverted
// table: DelDocs lose every posting (the changed page's old words, :455-531), the (DelTerm[i], DelDoc[i]) postings go
// (anchor words of its children, :533-616), the (AddTerm[i], AddDoc[i], AddW[i]) postings arrive.
type Delta struct {
	DelDocs         []uint32
	DelTerm, DelDoc []uint32
	AddTerm, AddDoc []uint32
	AddW            []float32
	AddPosPtr       []uint64  // optional: positions of the new postings, AddPosPtr[len(AddTerm)+1] into AddPos
	AddPos          []float32 // listPos[1:] (parser.go:195-207)
}

// ApplyDelta merges d into the resident table on the device (no BadgerDB row rewrite, no re-upload).  Scorers on this
// table must be closed before and created again after; call RefreshMagnitudes or TfIdfBuild next, as
// start_crawl.go:176-177 re-runs UpdateTermWeights after every crawl.
//
// When the table's squared magnitudes are resident (after TfIdfBuild or RefreshMagnitudes) the delta keeps the magnitudes
// of the docs it touches up to date itself; ReadMagnitudes returns them for the forw[4] rows.  New words / new child
// pages: Resize first.
func (ix *Index) ApplyDelta(d Delta) {
	check(ix.ctx, C.ss_index_apply_delta_pos(ix.h, C.uint64_t(len(d.DelDocs)), u32p(d.DelDocs),
		C.uint64_t(len(d.DelTerm)), u32p(d.DelTerm), u32p(d.DelDoc),
		C.uint64_t(len(d.AddTerm)), u32p(d.AddTerm), u32p(d.AddDoc), f32p(d.AddW), u64p(d.AddPosPtr), f32p(d.AddPos)), "ss_index_apply_delta_pos")
	var nPost C.uint64_t
	check(ix.ctx, C.ss_index_get_info(ix.h, nil, nil, &nPost), "ss_index_get_info")
	ix.NPost = uint64(nPost)
}

// Resize grows the doc and / or term space of the resident table (ss_index_resize).
func (ix *Index) Resize(nDocs, nTerms uint64) {
	check(ix.ctx, C.ss_index_resize(ix.h, C.uint64_t(nDocs), C.uint64_t(nTerms)), "ss_index_resize")
	ix.NDocs, ix.NTerms = nDocs, nTerms
}

// ReadMagnitudes returns the magnitudes of docs as they stand on the device.
func (ix *Index) ReadMagnitudes(docs []uint32) []float64 {
	mag := make([]float64, len(docs))
	check(ix.ctx, C.ss_index_read_magnitudes(ix.h, C.uint64_t(len(docs)), u32p(docs), f64p(mag)), "ss_index_read_magnitudes")
	return mag
}
func (ix *Index) RefreshMagnitudes() []float64 {
	mag := make([]float64, ix.NDocs)
	check(ix.ctx, C.ss_index_refresh_magnitudes(ix.h, f64p(mag)), "ss_index_refresh_magnitudes")
	return mag
}
func (ix *Index) SetWeighted(mag []float64) {
	check(ix.ctx, C.ss_index_set_weighted(ix.h, f64p(mag)), "ss_index_set_weighted")
}

// BuildDocView builds the doc-major view of the table as it stands (ss_index_build_doc_view): which terms a doc holds, with their
// current weights.  A snapshot: TfIdfBuild, ApplyDelta and Resize free it.  8 bytes per posting + 8 per doc of device memory.
func (ix *Index) BuildDocView() {
	check(ix.ctx, C.ss_index_build_doc_view(ix.h), "ss_index_build_doc_view")
}
func (ix *Index) DropDocView() {
	check(ix.ctx, C.ss_index_drop_doc_view(ix.h), "ss_index_drop_doc_view")
}

// SigEmpty fills every slot of the signature of a doc without terms (SS_SIG_EMPTY); MaxSigSlots is the most slots a signature has.
const SigEmpty = uint32(C.SS_SIG_EMPTY)
const MaxSigSlots = int(C.SS_MAX_SIG_SLOTS)

// BuildSignatures builds a MinHash signature of nSlots (4, 8, .., 32) words per doc from the doc view's term sets
// (ss_index_build_signatures; needs BuildDocView).  A snapshot of its own: TfIdfBuild, ApplyDelta and Resize free it, dropping the
// view does not.  4*nSlots bytes per doc of device memory.
func (ix *Index) BuildSignatures(nSlots int) {
	check(ix.ctx, C.ss_index_build_signatures(ix.h, C.int32_t(nSlots)), "ss_index_build_signatures")
}
func (ix *Index) DropSignatures() {
	check(ix.ctx, C.ss_index_drop_signatures(ix.h), "ss_index_drop_signatures")
}

// ReadSignatures returns the signature of every doc of docs, one row each.
func (ix *Index) ReadSignatures(docs []uint32) [][]uint32 {
	var nSlots C.int32_t
	check(ix.ctx, C.ss_index_read_signatures(ix.h, C.uint64_t(0), nil, nil, &nSlots), "ss_index_read_signatures")
	if len(docs) == 0 {
		return nil
	}
	s := int(nSlots)
	flat := make([]uint32, len(docs)*s)
	check(ix.ctx, C.ss_index_read_signatures(ix.h, C.uint64_t(len(docs)), u32p(docs), u32p(flat), nil), "ss_index_read_signatures")
	out := make([][]uint32, len(docs))
	for i := range docs {
		out[i] = flat[i*s : (i+1)*s]
	}
	return out
}

// DocTopTerms returns the m heaviest terms of every doc (weight descending, then term id; NaN last) and their weights:
// what the reference keeps per page as Words_mapping cut by sortMap (retrieval/util.go:116-149).  Needs BuildDocView.
func (ix *Index) DocTopTerms(docs []uint32, m int) ([][]uint32, [][]float32) {
	if len(docs) == 0 {
		return nil, nil
	}
	terms := make([]uint32, len(docs)*m)
	w := make([]float32, len(docs)*m)
	n := make([]int32, len(docs))
	check(ix.ctx, C.ss_index_doc_top_terms(ix.h, C.uint64_t(len(docs)), u32p(docs), C.int32_t(m), u32p(terms), f32p(w), i32p(n)),
		"ss_index_doc_top_terms")
	outT, outW := make([][]uint32, len(docs)), make([][]float32, len(docs))
	for i := range docs {
		outT[i] = terms[i*m : i*m+int(n[i])]
		outW[i] = w[i*m : i*m+int(n[i])]
	}
	return outT, outW
}

func (c *Ctx) NewScorer(title, body *Index) *Scorer {
	var h *C.ss_scorer
	check(c, C.ss_scorer_create(c.h, title.h, body.h, &h), "ss_scorer_create")
	var nDocs, nTerms, nPost C.uint64_t
	check(c, C.ss_index_get_info(title.h, &nDocs, &nTerms, &nPost), "ss_index_get_info")
	return &Scorer{h: h, ctx: c, nDocs: uint64(nDocs)}
}
func (s *Scorer) Close() { C.ss_scorer_destroy(s.h) }
func (s *Scorer) SetPrior(kTopics int, rank []float64) {
	check(s.ctx, C.ss_scorer_set_prior(s.h, C.int32_t(kTopics), f64p(rank)), "ss_scorer_set_prior")
}

// SetDocMasks registers allow-lists: words [nMasks][(nDocs+31)/32], bit (d & 31) of word d >> 5 = doc d allowed (nil clears).
func (s *Scorer) SetDocMasks(nMasks int, words []uint32) {
	check(s.ctx, C.ss_scorer_set_doc_masks(s.h, C.int32_t(nMasks), u32p(words)), "ss_scorer_set_doc_masks")
	s.nMasks = nMasks
	if len(words) == 0 {
		s.nMasks = 0
	}
}

// ScoreTopKMasked = ScoreTopKPhrase with one allow-list per query: maskID[q] (-1 = the whole index; nil = all -1); pPtr nil = no
// phrases.  Row q holds the first k docs of query q's ranking that its mask allows.
func (s *Scorer) ScoreTopKMasked(qPtr, qTerms, pPtr, pTerms []uint32, queryLen []int32, topicProbs []float64, maskID []int32, k int) ([][]Hit, error) {
	nq := len(qPtr) - 1
	if nq == 0 {
		return nil, nil
	}
	raw := make([]C.ss_hit, nq*k)
	nHits := make([]int32, nq)
	rc := C.ss_score_topk_masked(s.h, C.int32_t(nq), u32p(qPtr), u32p(qTerms), u32p(pPtr), u32p(pTerms), i32p(queryLen),
		f64p(topicProbs), i32p(maskID), C.int32_t(k), (*C.ss_hit)(unsafe.Pointer(&raw[0])), i32p(nHits))
	if err := statusErr(s.ctx, rc, "ss_score_topk_masked"); err != nil {
		return nil, err
	}
	out := make([][]Hit, nq)
	for q := 0; q < nq; q++ {
		out[q] = make([]Hit, nHits[q])
		for i := range out[q] {
			r := raw[q*k+i]
			out[q][i] = Hit{uint32(r.doc), float64(r.title), float64(r.body), float64(r.pagerank), float64(r.final)}
		}
	}
	return out, nil
}

// SimilarTopK answers "similar pages": row q = the top k of the query made of seed doc q's m heaviest body terms, without the seed
// itself (ss_similar_topk).  maskID as in ScoreTopKMasked (nil = none).  The body table needs its doc view (Index.BuildDocView).
func (s *Scorer) SimilarTopK(seeds []uint32, m int, topicProbs []float64, maskID []int32, k int) ([][]Hit, error) {
	nq := len(seeds)
	if nq == 0 {
		return nil, nil
	}
	raw := make([]C.ss_hit, nq*k)
	nHits := make([]int32, nq)
	rc := C.ss_similar_topk(s.h, C.int32_t(nq), u32p(seeds), C.int32_t(m), f64p(topicProbs), i32p(maskID), C.int32_t(k),
		(*C.ss_hit)(unsafe.Pointer(&raw[0])), i32p(nHits))
	if err := statusErr(s.ctx, rc, "ss_similar_topk"); err != nil {
		return nil, err
	}
	out := make([][]Hit, nq)
	for q := 0; q < nq; q++ {
		out[q] = make([]Hit, nHits[q])
		for i := range out[q] {
			r := raw[q*k+i]
			out[q][i] = Hit{uint32(r.doc), float64(r.title), float64(r.body), float64(r.pagerank), float64(r.final)}
		}
	}
	return out, nil
}

// RelatedTerm is one refinement word of RelatedTerms: a dense term id and the float64 sum of its weights over the feedback pages.
type RelatedTerm struct {
	Term  uint32
	Score float64
}

// RelatedTerms answers "which words do this query's best pages have in common that the user did not type?" (ss_related_terms): row q
// = up to m terms among the mDoc heaviest body terms of the query's kFb best pages, their weights summed per term in rank order, the
// query's own terms left out; score descending, then term id.  queryLen / topicProbs / maskID as in ScoreTopKMasked (nil = none).
// The body table needs its doc view (Index.BuildDocView).
func (s *Scorer) RelatedTerms(qPtr, qTerms []uint32, queryLen []int32, topicProbs []float64, maskID []int32, kFb, mDoc, m int) ([][]RelatedTerm, error) {
	nq := len(qPtr) - 1
	if nq <= 0 {
		return nil, nil
	}
	terms := make([]uint32, nq*m)
	score := make([]float64, nq*m)
	nOut := make([]int32, nq)
	rc := C.ss_related_terms(s.h, C.int32_t(nq), u32p(qPtr), u32p(qTerms), i32p(queryLen), f64p(topicProbs), i32p(maskID),
		C.int32_t(kFb), C.int32_t(mDoc), C.int32_t(m), u32p(terms), f64p(score), i32p(nOut))
	if err := statusErr(s.ctx, rc, "ss_related_terms"); err != nil {
		return nil, err
	}
	out := make([][]RelatedTerm, nq)
	for q := 0; q < nq; q++ {
		out[q] = make([]RelatedTerm, nOut[q])
		for i := range out[q] {
			out[q][i] = RelatedTerm{terms[q*m+i], score[q*m+i]}
		}
	}
	return out, nil
}

// TermMatch says how one query token matched one hit (ss_term_match): the stored weights of the (term, doc) postings, which of them
// exist, and the earliest body position >= 0 (HasPos false: no positional postings, no body posting, or no such position).
type TermMatch struct {
	TitleW  float32
	BodyW   float32
	InTitle bool
	InBody  bool
	HasPos  bool
	BodyPos float32
}

// ExplainHits answers "which of the query's tokens matched each result, and where?" (ss_explain_hits) for rows any scoring call
// returned: out[q][j][i] describes hits[q][j] and token i of query q (qTerms[qPtr[q]+i]; duplicates get equal entries).  Only the
// hits' Doc is read.  Unknown terms and doc ids the index does not hold match nothing.
func (s *Scorer) ExplainHits(qPtr, qTerms []uint32, hits [][]Hit) ([][][]TermMatch, error) {
	nq := len(qPtr) - 1
	if nq <= 0 || len(hits) != nq {
		return nil, nil
	}
	k, stride := 1, 1
	for q := 0; q < nq; q++ {
		if len(hits[q]) > k {
			k = len(hits[q])
		}
		if n := int(qPtr[q+1] - qPtr[q]); n > stride {
			stride = n
		}
	}
	raw := make([]C.ss_hit, nq*k)
	nHits := make([]int32, nq)
	for q := 0; q < nq; q++ {
		nHits[q] = int32(len(hits[q]))
		for j, h := range hits[q] {
			raw[q*k+j].doc = C.uint32_t(h.Doc)
		}
	}
	m := make([]C.ss_term_match, nq*k*stride)
	rc := C.ss_explain_hits(s.h, C.int32_t(nq), u32p(qPtr), u32p(qTerms), C.int32_t(k), (*C.ss_hit)(unsafe.Pointer(&raw[0])),
		i32p(nHits), C.int32_t(stride), (*C.ss_term_match)(unsafe.Pointer(&m[0])))
	if err := statusErr(s.ctx, rc, "ss_explain_hits"); err != nil {
		return nil, err
	}
	out := make([][][]TermMatch, nq)
	for q := 0; q < nq; q++ {
		nt := int(qPtr[q+1] - qPtr[q])
		out[q] = make([][]TermMatch, len(hits[q]))
		for j := range out[q] {
			out[q][j] = make([]TermMatch, nt)
			for i := 0; i < nt; i++ {
				e := m[(q*k+j)*stride+i]
				out[q][j][i] = TermMatch{float32(e.title_w), float32(e.body_w), e.flags&1 != 0, e.flags&2 != 0, e.flags&4 != 0, float32(e.body_pos)}
			}
		}
	}
	return out, nil
}

// Passage is the best body window of one hit (ss_passage): Start and Last are the position values of its first and last occurrence,
// Distinct the distinct query terms and Occurrences the occurrences inside it; bit i of TokenMask: the query's i-th token's term
// occurs in it.  Occurrences == 0: the doc has no passage.
type Passage struct {
	Start       float32
	Last        float32
	Distinct    uint32
	Occurrences uint32
	TokenMask   uint64
}

// BestPassages answers "where should each result's snippet start?" (ss_best_passages) for rows any scoring call returned:
// out[q][j] is the window of width body positions of hits[q][j] that holds most distinct terms of query q, then most occurrences,
// then starts earliest.  Only the hits' Doc is read.  Unknown terms and doc ids the index does not hold have no occurrences.
func (s *Scorer) BestPassages(qPtr, qTerms []uint32, hits [][]Hit, width int) ([][]Passage, error) {
	nq := len(qPtr) - 1
	if nq <= 0 || len(hits) != nq {
		return nil, nil
	}
	k := 1
	for q := 0; q < nq; q++ {
		if len(hits[q]) > k {
			k = len(hits[q])
		}
	}
	raw := make([]C.ss_hit, nq*k)
	nHits := make([]int32, nq)
	for q := 0; q < nq; q++ {
		nHits[q] = int32(len(hits[q]))
		for j, h := range hits[q] {
			raw[q*k+j].doc = C.uint32_t(h.Doc)
		}
	}
	m := make([]C.ss_passage, nq*k)
	rc := C.ss_best_passages(s.h, C.int32_t(nq), u32p(qPtr), u32p(qTerms), C.int32_t(k), (*C.ss_hit)(unsafe.Pointer(&raw[0])),
		i32p(nHits), C.int32_t(width), (*C.ss_passage)(unsafe.Pointer(&m[0])))
	if err := statusErr(s.ctx, rc, "ss_best_passages"); err != nil {
		return nil, err
	}
	out := make([][]Passage, nq)
	for q := 0; q < nq; q++ {
		out[q] = make([]Passage, len(hits[q]))
		for j := range out[q] {
			e := m[q*k+j]
			out[q][j] = Passage{float32(e.start), float32(e.last), uint32(e.n_distinct), uint32(e.n_occ), uint64(e.token_mask)}
		}
	}
	return out, nil
}

// Proximity is the smallest body span of one hit that holds every query term the doc has at all (ss_proximity): Start and End are
// the position values of its first and last occurrence, Present the distinct query terms the doc has and Occurrences the occurrences
// inside the span; bit i of TokenMask: the query's i-th token's term is present.  Present == 0: the doc holds none of the terms.
type Proximity struct {
	Start       float32
	End         float32
	Present     uint32
	Occurrences uint32
	TokenMask   uint64
}

// HitProximity answers "how close do the query's words come in each result?" (ss_hit_proximity) for rows any scoring call returned.
// Only the hits' Doc is read.  Unknown terms and doc ids the index does not hold have no occurrences.
func (s *Scorer) HitProximity(qPtr, qTerms []uint32, hits [][]Hit) ([][]Proximity, error) {
	nq := len(qPtr) - 1
	if nq <= 0 || len(hits) != nq {
		return nil, nil
	}
	k := 1
	for q := 0; q < nq; q++ {
		if len(hits[q]) > k {
			k = len(hits[q])
		}
	}
	raw := make([]C.ss_hit, nq*k)
	nHits := make([]int32, nq)
	for q := 0; q < nq; q++ {
		nHits[q] = int32(len(hits[q]))
		for j, h := range hits[q] {
			raw[q*k+j].doc = C.uint32_t(h.Doc)
		}
	}
	m := make([]C.ss_proximity, nq*k)
	rc := C.ss_hit_proximity(s.h, C.int32_t(nq), u32p(qPtr), u32p(qTerms), C.int32_t(k), (*C.ss_hit)(unsafe.Pointer(&raw[0])),
		i32p(nHits), (*C.ss_proximity)(unsafe.Pointer(&m[0])))
	if err := statusErr(s.ctx, rc, "ss_hit_proximity"); err != nil {
		return nil, err
	}
	out := make([][]Proximity, nq)
	for q := 0; q < nq; q++ {
		out[q] = make([]Proximity, len(hits[q]))
		for j := range out[q] {
			e := m[q*k+j]
			out[q][j] = Proximity{float32(e.start), float32(e.end), uint32(e.n_present), uint32(e.n_occ), uint64(e.token_mask)}
		}
	}
	return out, nil
}

// ProximityPage is one page of a query's results re-ranked by term proximity: Scores[i] = wRank * Final + wProx * bonus of Hits[i],
// Spans[i] its Proximity.
type ProximityPage struct {
	Hits   []Hit
	Scores []float64
	Spans  []Proximity
}

// ScoreTopKProximity = ScoreTopKMasked without phrases at k = kWindow, then the window sorted stably by wRank * Final + wProx * bonus,
// descending, and page [first, first+k) of it, in one library call: the window never leaves the device (ss_score_topk_proximity).
// bonus: how close the query's terms come in the doc's body, times the share of the query's terms the doc has.  maskID nil = none.
func (s *Scorer) ScoreTopKProximity(qPtr, qTerms []uint32, queryLen []int32, topicProbs []float64, maskID []int32, kWindow int,
	wRank, wProx float64, first, k int) ([]ProximityPage, error) {
	nq := len(qPtr) - 1
	if nq <= 0 {
		return nil, nil
	}
	kk := k
	if kk < 1 {
		kk = 1
	}
	raw := make([]C.ss_hit, nq*kk)
	nHits, scores, m := make([]int32, nq), make([]float64, nq*kk), make([]C.ss_proximity, nq*kk)
	rc := C.ss_score_topk_proximity(s.h, C.int32_t(nq), u32p(qPtr), u32p(qTerms), i32p(queryLen), f64p(topicProbs), i32p(maskID),
		C.int32_t(kWindow), C.double(wRank), C.double(wProx), C.int32_t(first), C.int32_t(k), (*C.ss_hit)(unsafe.Pointer(&raw[0])),
		i32p(nHits), f64p(scores), (*C.ss_proximity)(unsafe.Pointer(&m[0])))
	if err := statusErr(s.ctx, rc, "ss_score_topk_proximity"); err != nil {
		return nil, err
	}
	out := make([]ProximityPage, nq)
	for q := 0; q < nq; q++ {
		n := int(nHits[q])
		out[q] = ProximityPage{make([]Hit, n), append([]float64(nil), scores[q*kk:q*kk+n]...), make([]Proximity, n)}
		for i := 0; i < n; i++ {
			r, e := raw[q*kk+i], m[q*kk+i]
			out[q].Hits[i] = Hit{uint32(r.doc), float64(r.title), float64(r.body), float64(r.pagerank), float64(r.final)}
			out[q].Spans[i] = Proximity{float32(e.start), float32(e.end), uint32(e.n_present), uint32(e.n_occ), uint64(e.token_mask)}
		}
	}
	return out, nil
}

// RankNFeatures is the number of columns of HitFeatures (SS_RANK_N_FEATURES): title, body, pagerank, final, window position, query
// length, present terms, span, prox, occurrences, vector score, fields 0..3.  An absent signal is NaN.
const RankNFeatures = 15

// TreeNode is one node of a RankModel tree (ss_tree_node): Feature >= 0 splits on that column (left iff x <= Value, a NaN x left iff
// NanLeft), Feature -1 is a leaf whose output is Value.  Left and Right are indices inside the tree, larger than the node's own.
type TreeNode struct {
	Feature     int32
	Left, Right uint32
	NanLeft     bool
	Value       float64
}

// RankModel is a tree ensemble over feature rows (ss_rank_model): score(x) = base + the linear part over the non-NaN columns + the
// leaf every tree sends x to, added in tree order.
type RankModel struct {
	h         *C.ss_rank_model
	ctx       *Ctx
	nFeatures int
}

// NewRankModel uploads a trained model; the library validates all of it (children behind their parent and inside the tree, finite leaf
// values, ...) and an invalid one is an error.  linear nil = no linear part; trees may be empty (a linear model).
func (c *Ctx) NewRankModel(nFeatures int, linear []float64, base float64, trees [][]TreeNode) (*RankModel, error) {
	if linear != nil && len(linear) != nFeatures {
		return nil, fmt.Errorf("NewRankModel: %d linear weights for %d features", len(linear), nFeatures)
	}
	treePtr := make([]uint32, len(trees)+1)
	var nodes []C.ss_tree_node
	for t, tr := range trees {
		for _, n := range tr {
			var nl C.uint32_t
			if n.NanLeft {
				nl = 1
			}
			nodes = append(nodes, C.ss_tree_node{feature: C.int32_t(n.Feature), left: C.uint32_t(n.Left), right: C.uint32_t(n.Right),
				nan_left: nl, value: C.double(n.Value)})
		}
		treePtr[t+1] = uint32(len(nodes))
	}
	var np *C.ss_tree_node
	if len(nodes) > 0 {
		np = &nodes[0]
	}
	m := &RankModel{ctx: c, nFeatures: nFeatures}
	rc := C.ss_rank_model_create(c.h, C.int32_t(nFeatures), f64p(linear), C.double(base), C.int32_t(len(trees)), u32p(treePtr), np, &m.h)
	if err := statusErr(c, rc, "ss_rank_model_create"); err != nil {
		return nil, err
	}
	return m, nil
}

func (m *RankModel) Close() { C.ss_rank_model_destroy(m.h) }

// Eval scores feature rows x [nRows][nFeatures] (row-major) -> [nRows] (ss_rank_model_eval).
func (m *RankModel) Eval(x []float64) ([]float64, error) {
	if m.nFeatures == 0 || len(x)%m.nFeatures != 0 {
		return nil, fmt.Errorf("RankModel.Eval: %d values are not whole rows of %d features", len(x), m.nFeatures)
	}
	n := len(x) / m.nFeatures
	out := make([]float64, n)
	if n == 0 {
		return out, nil
	}
	rc := C.ss_rank_model_eval(m.h, C.int64_t(n), f64p(x), f64p(out))
	return out, statusErr(m.ctx, rc, "ss_rank_model_eval")
}

// windowOf packs per-query rows into the [nq][k] layout the window calls take.
func windowOf(hits [][]Hit) ([]C.ss_hit, []int32, int) {
	k := 1
	for _, row := range hits {
		if len(row) > k {
			k = len(row)
		}
	}
	raw := make([]C.ss_hit, len(hits)*k)
	nHits := make([]int32, len(hits))
	for q, row := range hits {
		nHits[q] = int32(len(row))
		for j, h := range row {
			raw[q*k+j] = C.ss_hit{doc: C.uint32_t(h.Doc), title: C.double(h.Title), body: C.double(h.Body), pagerank: C.double(h.PageRank),
				final: C.double(h.Final)}
		}
	}
	return raw, nHits, k
}

// windowExtras packs the optional per-row inputs of HitFeatures / RerankByModel (nil = absent) beside a window of width k.
func windowExtras(hits [][]Hit, k int, prox [][]Proximity, vecScores [][]int32) ([]C.ss_proximity, []int32) {
	var px []C.ss_proximity
	var vs []int32
	if prox != nil {
		px = make([]C.ss_proximity, len(hits)*k)
		for q := range hits {
			for j := 0; j < len(hits[q]) && j < len(prox[q]); j++ {
				e := prox[q][j]
				px[q*k+j] = C.ss_proximity{start: C.float(e.Start), end: C.float(e.End), n_present: C.uint32_t(e.Present),
					n_occ: C.uint32_t(e.Occurrences), token_mask: C.uint64_t(e.TokenMask)}
			}
		}
	}
	if vecScores != nil {
		vs = make([]int32, len(hits)*k)
		for q := range hits {
			copy(vs[q*k:q*k+k], vecScores[q])
		}
	}
	return px, vs
}

// HitFeatures assembles the signals of every row into a feature row (ss_hit_features): out[q][j] holds RankNFeatures values for
// hits[q][j].  prox as HitProximity returns it, vecScores as HitVectorScores, queryLen one value per query; nil = that signal is absent.
func (s *Scorer) HitFeatures(hits [][]Hit, prox [][]Proximity, vecScores [][]int32, queryLen []int32) ([][][]float64, error) {
	nq := len(hits)
	if nq == 0 {
		return nil, nil
	}
	raw, nHits, k := windowOf(hits)
	px, vs := windowExtras(hits, k, prox, vecScores)
	var pp *C.ss_proximity
	if px != nil {
		pp = &px[0]
	}
	flat := make([]float64, nq*k*RankNFeatures)
	rc := C.ss_hit_features(s.h, C.int32_t(nq), C.int32_t(k), &raw[0], i32p(nHits), pp, i32p(vs), i32p(queryLen), f64p(flat))
	if err := statusErr(s.ctx, rc, "ss_hit_features"); err != nil {
		return nil, err
	}
	out := make([][][]float64, nq)
	for q := range hits {
		out[q] = make([][]float64, len(hits[q]))
		for j := range out[q] {
			at := (q*k + j) * RankNFeatures
			out[q][j] = flat[at : at+RankNFeatures : at+RankNFeatures]
		}
	}
	return out, nil
}

// RankedPage is one page of a query's results re-ranked by a model: Scores[i] = the model's score of Hits[i]'s feature row.
type RankedPage struct {
	Hits   []Hit
	Scores []float64
}

// RerankByModel sorts every window stably by the model's score of each row's HitFeatures entry, descending (NaN scores behind every
// number, rows outside the table last), and returns page [first, first+k) (ss_rerank_hits_by_model).  The model must read
// RankNFeatures columns.  prox, vecScores, queryLen as in HitFeatures.
func (s *Scorer) RerankByModel(m *RankModel, hits [][]Hit, prox [][]Proximity, vecScores [][]int32, queryLen []int32,
	first, k int) ([]RankedPage, error) {
	nq := len(hits)
	if nq == 0 {
		return nil, nil
	}
	raw, nHits, kIn := windowOf(hits)
	px, vs := windowExtras(hits, kIn, prox, vecScores)
	var pp *C.ss_proximity
	if px != nil {
		pp = &px[0]
	}
	kk := k
	if kk < 1 {
		kk = 1
	}
	page := make([]C.ss_hit, nq*kk)
	nPage, scores := make([]int32, nq), make([]float64, nq*kk)
	rc := C.ss_rerank_hits_by_model(s.h, m.h, C.int32_t(nq), C.int32_t(kIn), &raw[0], i32p(nHits), pp, i32p(vs), i32p(queryLen),
		C.int32_t(first), C.int32_t(k), &page[0], i32p(nPage), f64p(scores))
	if err := statusErr(s.ctx, rc, "ss_rerank_hits_by_model"); err != nil {
		return nil, err
	}
	out := make([]RankedPage, nq)
	for q := 0; q < nq; q++ {
		n := int(nPage[q])
		out[q] = RankedPage{make([]Hit, n), append([]float64(nil), scores[q*kk:q*kk+n]...)}
		for i := 0; i < n; i++ {
			r := page[q*kk+i]
			out[q].Hits[i] = Hit{uint32(r.doc), float64(r.title), float64(r.body), float64(r.pagerank), float64(r.final)}
		}
	}
	return out, nil
}

// NoGroup in a group table: the doc is never collapsed with anything (SS_NO_GROUP).
const NoGroup = uint32(C.SS_NO_GROUP)

// SetDocGroups registers the doc -> group table for collapsed result pages: group[d] = the site of doc d (any 32-bit value),
// NoGroup = never collapsed; one entry per doc of the scorer (nil clears).
func (s *Scorer) SetDocGroups(group []uint32) {
	check(s.ctx, C.ss_scorer_set_doc_groups(s.h, u32p(group)), "ss_scorer_set_doc_groups")
}

// CollapsedPage is one page of a query's results with at most g rows per group: Same[i] = rows of the whole window in the group of
// Hits[i], the row itself included; Kept = rows the whole window keeps.
type CollapsedPage struct {
	Hits []Hit
	Same []uint32
	Kept int
}

func collapsedPages(nq, k int, raw []C.ss_hit, nHits []int32, same []uint32, kept []int32) []CollapsedPage {
	out := make([]CollapsedPage, nq)
	for q := 0; q < nq; q++ {
		n := int(nHits[q])
		out[q] = CollapsedPage{make([]Hit, n), append([]uint32(nil), same[q*k:q*k+n]...), int(kept[q])}
		for i := 0; i < n; i++ {
			r := raw[q*k+i]
			out[q].Hits[i] = Hit{uint32(r.doc), float64(r.title), float64(r.body), float64(r.pagerank), float64(r.final)}
		}
	}
	return out
}

// CollapseHits keeps at most g rows per group of every window hits[q], in the order given (ss_collapse_hits), and returns page
// [first, first+k) of the kept rows.  The rows may come from any scoring call; needs SetDocGroups.
func (s *Scorer) CollapseHits(hits [][]Hit, g, first, k int) ([]CollapsedPage, error) {
	nq := len(hits)
	if nq == 0 {
		return nil, nil
	}
	kIn := 1
	for q := 0; q < nq; q++ {
		if len(hits[q]) > kIn {
			kIn = len(hits[q])
		}
	}
	in := make([]C.ss_hit, nq*kIn)
	nIn := make([]int32, nq)
	for q := 0; q < nq; q++ {
		nIn[q] = int32(len(hits[q]))
		for j, h := range hits[q] {
			in[q*kIn+j] = C.ss_hit{doc: C.uint32_t(h.Doc), title: C.double(h.Title), body: C.double(h.Body), pagerank: C.double(h.PageRank),
				final: C.double(h.Final)}
		}
	}
	kk := k
	if kk < 1 {
		kk = 1
	}
	raw := make([]C.ss_hit, nq*kk)
	nHits, kept, same := make([]int32, nq), make([]int32, nq), make([]uint32, nq*kk)
	rc := C.ss_collapse_hits(s.h, C.int32_t(nq), C.int32_t(kIn), (*C.ss_hit)(unsafe.Pointer(&in[0])), i32p(nIn), C.int32_t(g),
		C.int32_t(first), C.int32_t(k), (*C.ss_hit)(unsafe.Pointer(&raw[0])), i32p(nHits), u32p(same), i32p(kept))
	if err := statusErr(s.ctx, rc, "ss_collapse_hits"); err != nil {
		return nil, err
	}
	return collapsedPages(nq, kk, raw, nHits, same, kept), nil
}

// ScoreTopKCollapsed = ScoreTopKMasked without phrases at k = kWindow, then CollapseHits on its rows, in one library call: the window
// never leaves the device (ss_score_topk_collapsed).  maskID nil = none.
func (s *Scorer) ScoreTopKCollapsed(qPtr, qTerms []uint32, queryLen []int32, topicProbs []float64, maskID []int32, kWindow, g, first,
	k int) ([]CollapsedPage, error) {
	nq := len(qPtr) - 1
	if nq <= 0 {
		return nil, nil
	}
	kk := k
	if kk < 1 {
		kk = 1
	}
	raw := make([]C.ss_hit, nq*kk)
	nHits, kept, same := make([]int32, nq), make([]int32, nq), make([]uint32, nq*kk)
	rc := C.ss_score_topk_collapsed(s.h, C.int32_t(nq), u32p(qPtr), u32p(qTerms), i32p(queryLen), f64p(topicProbs), i32p(maskID),
		C.int32_t(kWindow), C.int32_t(g), C.int32_t(first), C.int32_t(k), (*C.ss_hit)(unsafe.Pointer(&raw[0])), i32p(nHits), u32p(same),
		i32p(kept))
	if err := statusErr(s.ctx, rc, "ss_score_topk_collapsed"); err != nil {
		return nil, err
	}
	return collapsedPages(nq, kk, raw, nHits, same, kept), nil
}

// DedupedPage is one page of a query's results without near-duplicate rows: Similar[i] = rows of the whole window that Hits[i] leads,
// itself included ("Similar[i]-1 very similar results omitted"); Kept = rows the whole window keeps.
type DedupedPage struct {
	Hits    []Hit
	Similar []uint32
	Kept    int
}

// DedupHits drops from every window hits[q], in the order given, the rows whose body signature agrees in at least minMatch slots
// with an earlier kept row's (ss_dedup_hits), and returns page [first, first+k) of the kept rows.  The rows may come from any
// scoring call; the body table needs BuildSignatures.
func (s *Scorer) DedupHits(hits [][]Hit, minMatch, first, k int) ([]DedupedPage, error) {
	nq := len(hits)
	if nq == 0 {
		return nil, nil
	}
	kIn := 1
	for q := 0; q < nq; q++ {
		if len(hits[q]) > kIn {
			kIn = len(hits[q])
		}
	}
	in := make([]C.ss_hit, nq*kIn)
	nIn := make([]int32, nq)
	for q := 0; q < nq; q++ {
		nIn[q] = int32(len(hits[q]))
		for j, h := range hits[q] {
			in[q*kIn+j] = C.ss_hit{doc: C.uint32_t(h.Doc), title: C.double(h.Title), body: C.double(h.Body), pagerank: C.double(h.PageRank),
				final: C.double(h.Final)}
		}
	}
	kk := k
	if kk < 1 {
		kk = 1
	}
	raw := make([]C.ss_hit, nq*kk)
	nHits, kept, similar := make([]int32, nq), make([]int32, nq), make([]uint32, nq*kk)
	rc := C.ss_dedup_hits(s.h, C.int32_t(nq), C.int32_t(kIn), (*C.ss_hit)(unsafe.Pointer(&in[0])), i32p(nIn), C.int32_t(minMatch),
		C.int32_t(first), C.int32_t(k), (*C.ss_hit)(unsafe.Pointer(&raw[0])), i32p(nHits), u32p(similar), i32p(kept))
	if err := statusErr(s.ctx, rc, "ss_dedup_hits"); err != nil {
		return nil, err
	}
	pages := collapsedPages(nq, kk, raw, nHits, similar, kept)
	out := make([]DedupedPage, nq)
	for q, p := range pages {
		out[q] = DedupedPage{p.Hits, p.Same, p.Kept}
	}
	return out, nil
}

// DocRange is one range clause over the doc fields (ss_doc_range): it matches doc d iff Lo <= value[Field][d] <= Hi.
type DocRange struct {
	Field  int32
	Lo, Hi int64
}

func docRanges(rng []DocRange) (*C.ss_doc_range, []C.ss_doc_range) {
	if len(rng) == 0 {
		return nil, nil
	}
	raw := make([]C.ss_doc_range, len(rng))
	for i, r := range rng {
		raw[i].field, raw[i].lo, raw[i].hi = C.int32_t(r.Field), C.int64_t(r.Lo), C.int64_t(r.Hi)
	}
	return (*C.ss_doc_range)(unsafe.Pointer(&raw[0])), raw
}

func i64p(s []int64) *C.int64_t {
	if len(s) == 0 {
		return nil
	}
	return (*C.int64_t)(unsafe.Pointer(&s[0]))
}

// SetDocFields registers the per-doc field table (ss_scorer_set_doc_fields): values[f*nDocs+d] = field f of doc d, up to
// C.SS_MAX_DOC_FIELDS fields (the shim's convention: field 0 = Mod_date as unix seconds, field 1 = Page_size; retrieval/util.go:28-29).
// nFields 0 clears.  Register it again after an index update, like the allow-lists.  values must hold nFields * nDocs entries.
func (s *Scorer) SetDocFields(nFields int, values []int64) {
	if nFields > 0 && uint64(len(values)) < uint64(nFields)*s.nDocs {
		panic(fmt.Errorf("SetDocFields: %d values for %d fields of %d docs", len(values), nFields, s.nDocs))
	}
	check(s.ctx, C.ss_scorer_set_doc_fields(s.h, C.int32_t(nFields), i64p(values)), "ss_scorer_set_doc_fields")
	s.nFields = nFields
	if len(values) == 0 {
		s.nFields = 0
	}
}

// DocFieldMasks builds allow-lists from range clauses on the device (ss_doc_field_masks): set i = the registered allow-list maskID[i]
// (-1 / nil: every doc) AND every clause of rng[rngPtr[i]:rngPtr[i+1]].  The words come back in the layout SetDocMasks takes,
// (nDocs+31)/32 per set with the scorer's own doc count.
func (s *Scorer) DocFieldMasks(rngPtr []uint32, rng []DocRange, maskID []int32) ([]uint32, error) {
	nSets := len(rngPtr) - 1
	if nSets <= 0 {
		return nil, nil
	}
	words := make([]uint32, uint64(nSets)*((s.nDocs+31)/32))
	rp, keep := docRanges(rng)
	rc := C.ss_doc_field_masks(s.h, C.int32_t(nSets), u32p(rngPtr), rp, i32p(maskID), u32p(words))
	runtime.KeepAlive(keep)
	if err := statusErr(s.ctx, rc, "ss_doc_field_masks"); err != nil {
		return nil, err
	}
	return words, nil
}

// ScoreTopKFiltered = ScoreTopKConstrained plus range clauses per query over the doc fields (ss_score_topk_filtered): every result
// of query q also matches each clause of rng[rngPtr[q]:rngPtr[q+1]]; rngPtr nil = none.
func (s *Scorer) ScoreTopKFiltered(qPtr, qTerms, pPtr, pTerms []uint32, queryLen []int32, topicProbs []float64, maskID []int32,
	reqPtr, reqTerms, excPtr, excTerms, rngPtr []uint32, rng []DocRange, k int) ([][]Hit, error) {
	nq := len(qPtr) - 1
	if nq == 0 {
		return nil, nil
	}
	raw := make([]C.ss_hit, nq*k)
	nHits := make([]int32, nq)
	rp, keep := docRanges(rng)
	rc := C.ss_score_topk_filtered(s.h, C.int32_t(nq), u32p(qPtr), u32p(qTerms), u32p(pPtr), u32p(pTerms), i32p(queryLen),
		f64p(topicProbs), i32p(maskID), u32p(reqPtr), u32p(reqTerms), u32p(excPtr), u32p(excTerms), u32p(rngPtr), rp, C.int32_t(k),
		(*C.ss_hit)(unsafe.Pointer(&raw[0])), i32p(nHits))
	runtime.KeepAlive(keep)
	if err := statusErr(s.ctx, rc, "ss_score_topk_filtered"); err != nil {
		return nil, err
	}
	out := make([][]Hit, nq)
	for q := 0; q < nq; q++ {
		out[q] = make([]Hit, nHits[q])
		for i := range out[q] {
			r := raw[q*k+i]
			out[q][i] = Hit{uint32(r.doc), float64(r.title), float64(r.body), float64(r.pagerank), float64(r.final)}
		}
	}
	return out, nil
}

// FacetCount is one query's counts from FacetCounts: the docs it matches, those of them in every registered allow-list, and those whose
// field value lies in every bucket of the call.
type FacetCount struct {
	Total   uint32
	Masks   []uint32
	Buckets []uint32
}

// FacetCounts counts, per query, the docs ScoreTopKFiltered ranks for the same query terms, maskID, required / excluded terms and range
// clauses (no phrase form), how many of them every allow-list of SetDocMasks holds, and how many fall into every bucket
// (ss_facet_counts).  buckets are shared by the batch, at most C.SS_MAX_FACET_BUCKETS; nil pointer arrays = none, as in ScoreTopKFiltered.
func (s *Scorer) FacetCounts(qPtr, qTerms []uint32, maskID []int32, reqPtr, reqTerms, excPtr, excTerms, rngPtr []uint32, rng []DocRange,
	buckets []DocRange) ([]FacetCount, error) {
	nq := len(qPtr) - 1
	if nq <= 0 {
		return nil, nil
	}
	nm, nb := s.nMasks, len(buckets)
	total := make([]uint32, nq)
	byMask, byBucket := make([]uint32, nq*nm), make([]uint32, nq*nb)
	rp, keepR := docRanges(rng)
	bp, keepB := docRanges(buckets)
	rc := C.ss_facet_counts(s.h, C.int32_t(nq), u32p(qPtr), u32p(qTerms), i32p(maskID), u32p(reqPtr), u32p(reqTerms), u32p(excPtr),
		u32p(excTerms), u32p(rngPtr), rp, C.int32_t(nb), bp, u32p(total), u32p(byMask), u32p(byBucket))
	runtime.KeepAlive(keepR)
	runtime.KeepAlive(keepB)
	if err := statusErr(s.ctx, rc, "ss_facet_counts"); err != nil {
		return nil, err
	}
	out := make([]FacetCount, nq)
	for q := 0; q < nq; q++ {
		out[q] = FacetCount{total[q], byMask[q*nm : (q+1)*nm], byBucket[q*nb : (q+1)*nb]}
	}
	return out, nil
}

// FieldPage is one query's page from FieldTopK: the docs in field order, their values, and the number of docs the query matches in all.
type FieldPage struct {
	Docs    []uint32
	Values  []int64
	Matches uint32
}

// FieldTopK returns, per query, page [first, first+k) of ALL docs FacetCounts counts for the same arguments, ordered by a doc field,
// ascending or descending, docs of equal value by ascending doc id (ss_field_topk).  first + k may not exceed C.SS_MAX_TOPK.
func (s *Scorer) FieldTopK(qPtr, qTerms []uint32, maskID []int32, reqPtr, reqTerms, excPtr, excTerms, rngPtr []uint32, rng []DocRange,
	field int, descending bool, first, k int) ([]FieldPage, error) {
	nq := len(qPtr) - 1
	if nq <= 0 {
		return nil, nil
	}
	kk := k
	if kk < 1 {
		kk = 1
	}
	desc := 0
	if descending {
		desc = 1
	}
	docs, nOut := make([]uint32, nq*kk), make([]int32, nq)
	vals, nMatch := make([]int64, nq*kk), make([]uint32, nq)
	rp, keepR := docRanges(rng)
	rc := C.ss_field_topk(s.h, C.int32_t(nq), u32p(qPtr), u32p(qTerms), i32p(maskID), u32p(reqPtr), u32p(reqTerms), u32p(excPtr),
		u32p(excTerms), u32p(rngPtr), rp, C.int32_t(field), C.int32_t(desc), C.int32_t(first), C.int32_t(k), u32p(docs), i32p(nOut),
		i64p(vals), u32p(nMatch))
	runtime.KeepAlive(keepR)
	if err := statusErr(s.ctx, rc, "ss_field_topk"); err != nil {
		return nil, err
	}
	out := make([]FieldPage, nq)
	for q := 0; q < nq; q++ {
		n := int(nOut[q])
		out[q] = FieldPage{docs[q*kk : q*kk+n], vals[q*kk : q*kk+n], nMatch[q]}
	}
	return out, nil
}

// GroupCount is one row of TopGroups: a value of the doc -> group table and the number of the query's matches that carry it.
type GroupCount struct {
	Group uint32
	Count uint32
}

// GroupPage is one query's page from TopGroups: the groups in count order, the number of distinct groups among the matches, the matches
// without a group (SS_NO_GROUP) and the number of docs the query matches in all.
type GroupPage struct {
	Rows      []GroupCount
	Groups    uint32
	Ungrouped uint32
	Matches   uint32
}

// GroupValues returns the distinct values other than SS_NO_GROUP of the registered group table, ascending (ss_scorer_group_values).
func (s *Scorer) GroupValues() ([]uint32, error) {
	var n C.uint32_t
	if err := statusErr(s.ctx, C.ss_scorer_group_values(s.h, &n, nil), "ss_scorer_group_values"); err != nil {
		return nil, err
	}
	values := make([]uint32, int(n))
	if n == 0 {
		return values, nil
	}
	if err := statusErr(s.ctx, C.ss_scorer_group_values(s.h, nil, u32p(values)), "ss_scorer_group_values"); err != nil {
		return nil, err
	}
	return values, nil
}

// TopGroups returns, per query, page [first, first+m) of the groups (SetDocGroups) that hold docs FacetCounts counts for the same
// arguments, by the number of such docs descending, equal counts by ascending group value (ss_top_groups).  first + m may not exceed
// C.SS_MAX_TOPK.
func (s *Scorer) TopGroups(qPtr, qTerms []uint32, maskID []int32, reqPtr, reqTerms, excPtr, excTerms, rngPtr []uint32, rng []DocRange,
	first, m int) ([]GroupPage, error) {
	nq := len(qPtr) - 1
	if nq <= 0 {
		return nil, nil
	}
	mm := m
	if mm < 1 {
		mm = 1
	}
	rows, nOut := make([]C.ss_group_count, nq*mm), make([]int32, nq)
	nGroups, nUngrouped, nMatch := make([]uint32, nq), make([]uint32, nq), make([]uint32, nq)
	rp, keepR := docRanges(rng)
	rc := C.ss_top_groups(s.h, C.int32_t(nq), u32p(qPtr), u32p(qTerms), i32p(maskID), u32p(reqPtr), u32p(reqTerms), u32p(excPtr),
		u32p(excTerms), u32p(rngPtr), rp, C.int32_t(first), C.int32_t(m), &rows[0], i32p(nOut), u32p(nGroups), u32p(nUngrouped),
		u32p(nMatch))
	runtime.KeepAlive(keepR)
	if err := statusErr(s.ctx, rc, "ss_top_groups"); err != nil {
		return nil, err
	}
	out := make([]GroupPage, nq)
	for q := 0; q < nq; q++ {
		n := int(nOut[q])
		page := make([]GroupCount, n)
		for r := 0; r < n; r++ {
			page[r] = GroupCount{uint32(rows[q*mm+r].group), uint32(rows[q*mm+r].count)}
		}
		out[q] = GroupPage{page, nGroups[q], nUngrouped[q], nMatch[q]}
	}
	return out, nil
}

// FieldStat is one (query, field) entry of FieldStats: the smallest and largest value and the exact sum SumHi * 2^64 + SumLo (two's
// complement) over the Count matches that have a value, and the Missing matches whose value is SS_NO_FIELD_VALUE.  Count 0: Min
// math.MaxInt64, Max math.MinInt64.
type FieldStat struct {
	Min, Max int64
	SumLo    uint64
	SumHi    int64
	Count    uint32
	Missing  uint32
}

// FieldStatsRow is one query's entries from FieldStats, one per asked field, and the number of docs the query matches in all.
type FieldStatsRow struct {
	Fields  []FieldStat
	Matches uint32
}

// FieldStats returns, per query and per field of fields (at most C.SS_MAX_DOC_FIELDS, repeats allowed), the range, the exact sum and the
// missing count of the field over ALL docs FacetCounts counts for the same arguments (ss_field_stats).
func (s *Scorer) FieldStats(qPtr, qTerms []uint32, maskID []int32, reqPtr, reqTerms, excPtr, excTerms, rngPtr []uint32, rng []DocRange,
	fields []int32) ([]FieldStatsRow, error) {
	nq := len(qPtr) - 1
	if nq <= 0 {
		return nil, nil
	}
	nf := len(fields)
	stats, nMatch := make([]C.ss_field_stat, nq*nf+1), make([]uint32, nq)
	rp, keepR := docRanges(rng)
	rc := C.ss_field_stats(s.h, C.int32_t(nq), u32p(qPtr), u32p(qTerms), i32p(maskID), u32p(reqPtr), u32p(reqTerms), u32p(excPtr),
		u32p(excTerms), u32p(rngPtr), rp, C.int32_t(nf), i32p(fields), &stats[0], u32p(nMatch))
	runtime.KeepAlive(keepR)
	if err := statusErr(s.ctx, rc, "ss_field_stats"); err != nil {
		return nil, err
	}
	out := make([]FieldStatsRow, nq)
	for q := 0; q < nq; q++ {
		row := make([]FieldStat, nf)
		for i := 0; i < nf; i++ {
			r := stats[q*nf+i]
			row[i] = FieldStat{int64(r.min), int64(r.max), uint64(r.sum_lo), int64(r.sum_hi), uint32(r.count), uint32(r.missing)}
		}
		out[q] = FieldStatsRow{row, nMatch[q]}
	}
	return out, nil
}

// FieldHistogramRow is one query's bins from FieldHistogram: Counts per bin, the matches below the first bin, at or above the end of the
// last one and without a value, and the number of docs the query matches in all (the sum of the others).
type FieldHistogramRow struct {
	Counts  []uint32
	Below   uint32
	Above   uint32
	Missing uint32
	Matches uint32
}

// FieldHistogram counts, per query, the docs FacetCounts counts for the same arguments in every bin of a doc field (ss_field_histogram).
// edges nil: nBins bins of the given width (1 .. 2^64-1) from origin.  edges [nBins+1], strictly ascending: bin b holds
// edges[b] <= value < edges[b+1]; origin and width are ignored.  nBins may not exceed C.SS_MAX_HIST_BINS.
func (s *Scorer) FieldHistogram(qPtr, qTerms []uint32, maskID []int32, reqPtr, reqTerms, excPtr, excTerms, rngPtr []uint32, rng []DocRange,
	field int, origin int64, width uint64, edges []int64, nBins int) ([]FieldHistogramRow, error) {
	nq := len(qPtr) - 1
	if nq <= 0 {
		return nil, nil
	}
	if edges != nil && len(edges) < nBins+1 {
		return nil, fmt.Errorf("ss_field_histogram: %d edges for %d bins", len(edges), nBins)
	}
	nb := nBins
	if nb < 1 {
		nb = 1
	}
	counts, tails := make([]uint32, nq*nb), make([]C.ss_hist_tail, nq)
	rp, keepR := docRanges(rng)
	rc := C.ss_field_histogram(s.h, C.int32_t(nq), u32p(qPtr), u32p(qTerms), i32p(maskID), u32p(reqPtr), u32p(reqTerms), u32p(excPtr),
		u32p(excTerms), u32p(rngPtr), rp, C.int32_t(field), C.int64_t(origin), C.uint64_t(width), i64p(edges), C.int32_t(nBins),
		u32p(counts), &tails[0])
	runtime.KeepAlive(keepR)
	if err := statusErr(s.ctx, rc, "ss_field_histogram"); err != nil {
		return nil, err
	}
	out := make([]FieldHistogramRow, nq)
	for q := 0; q < nq; q++ {
		t := tails[q]
		out[q] = FieldHistogramRow{counts[q*nb : (q+1)*nb], uint32(t.below), uint32(t.above), uint32(t.missing), uint32(t.n_match)}
	}
	return out, nil
}

// SortHitsByField sorts every window stably by a doc field, ascending or descending, rows outside the table last, and returns page
// [first, first+k) with the rows' values (ss_sort_hits_by_field).  Only the hits' Doc is read to decide anything.
func (s *Scorer) SortHitsByField(hits [][]Hit, field int, descending bool, first, k int) ([][]Hit, [][]int64, error) {
	nq := len(hits)
	if nq == 0 {
		return nil, nil, nil
	}
	kIn := 1
	for q := 0; q < nq; q++ {
		if len(hits[q]) > kIn {
			kIn = len(hits[q])
		}
	}
	in := make([]C.ss_hit, nq*kIn)
	nIn := make([]int32, nq)
	for q := 0; q < nq; q++ {
		nIn[q] = int32(len(hits[q]))
		for j, h := range hits[q] {
			in[q*kIn+j] = C.ss_hit{doc: C.uint32_t(h.Doc), title: C.double(h.Title), body: C.double(h.Body), pagerank: C.double(h.PageRank),
				final: C.double(h.Final)}
		}
	}
	kk := k
	if kk < 1 {
		kk = 1
	}
	desc := 0
	if descending {
		desc = 1
	}
	raw := make([]C.ss_hit, nq*kk)
	nHits, vals := make([]int32, nq), make([]int64, nq*kk)
	rc := C.ss_sort_hits_by_field(s.h, C.int32_t(nq), C.int32_t(kIn), (*C.ss_hit)(unsafe.Pointer(&in[0])), i32p(nIn), C.int32_t(field),
		C.int32_t(desc), C.int32_t(first), C.int32_t(k), (*C.ss_hit)(unsafe.Pointer(&raw[0])), i32p(nHits), i64p(vals))
	if err := statusErr(s.ctx, rc, "ss_sort_hits_by_field"); err != nil {
		return nil, nil, err
	}
	out, outVals := make([][]Hit, nq), make([][]int64, nq)
	for q := 0; q < nq; q++ {
		n := int(nHits[q])
		out[q], outVals[q] = make([]Hit, n), append([]int64(nil), vals[q*kk:q*kk+n]...)
		for i := 0; i < n; i++ {
			r := raw[q*kk+i]
			out[q][i] = Hit{uint32(r.doc), float64(r.title), float64(r.body), float64(r.pagerank), float64(r.final)}
		}
	}
	return out, outVals, nil
}

// HitFields reads the field values of every hit (ss_hit_fields): out[q][j][f] for the fields SetDocFields registered;
// C.SS_NO_FIELD_VALUE for a doc outside the table.
func (s *Scorer) HitFields(hits [][]Hit) ([][][]int64, error) {
	nq, nFields := len(hits), s.nFields
	if nq == 0 {
		return nil, nil
	}
	if nFields < 1 {
		return nil, fmt.Errorf("HitFields: no doc fields registered (SetDocFields)")
	}
	kIn := 1
	for q := 0; q < nq; q++ {
		if len(hits[q]) > kIn {
			kIn = len(hits[q])
		}
	}
	in := make([]C.ss_hit, nq*kIn)
	nIn := make([]int32, nq)
	for q := 0; q < nq; q++ {
		nIn[q] = int32(len(hits[q]))
		for j, h := range hits[q] {
			in[q*kIn+j].doc = C.uint32_t(h.Doc)
		}
	}
	vals := make([]int64, nq*kIn*nFields)
	rc := C.ss_hit_fields(s.h, C.int32_t(nq), C.int32_t(kIn), (*C.ss_hit)(unsafe.Pointer(&in[0])), i32p(nIn), i64p(vals))
	if err := statusErr(s.ctx, rc, "ss_hit_fields"); err != nil {
		return nil, err
	}
	out := make([][][]int64, nq)
	for q := 0; q < nq; q++ {
		out[q] = make([][]int64, len(hits[q]))
		for j := range out[q] {
			o := (q*kIn + j) * nFields
			out[q][j] = append([]int64(nil), vals[o:o+nFields]...)
		}
	}
	return out, nil
}

func i8p(s []int8) *C.int8_t {
	if len(s) == 0 {
		return nil
	}
	return (*C.int8_t)(unsafe.Pointer(&s[0]))
}

// VecHit is one row of VectorTopK: a doc and its exact integer dot product with the query vector.
type VecHit struct {
	Doc   uint32
	Score int32
}

// SetDocVectors registers one int8 vector per doc (ss_scorer_set_doc_vectors): vec[d*dim+i] = position i of doc d, dim a multiple
// of 64 up to C.SS_MAX_VEC_DIM.  dim 0 clears.  Register it again after an index update, like the allow-lists.
func (s *Scorer) SetDocVectors(dim int, vec []int8) {
	if dim > 0 && uint64(len(vec)) < uint64(dim)*s.nDocs {
		panic(fmt.Errorf("SetDocVectors: %d values for %d docs of dim %d", len(vec), s.nDocs, dim))
	}
	check(s.ctx, C.ss_scorer_set_doc_vectors(s.h, C.int32_t(dim), i8p(vec)), "ss_scorer_set_doc_vectors")
	s.vecDim = dim
	s.nVecLists = 0 // (the library drops the lists: they describe the old table)
	if len(vec) == 0 {
		s.vecDim = 0
	}
}

// VectorTopK returns per query vector (qvec[q*dim:(q+1)*dim]) the exact k nearest docs by integer dot product, score descending
// then doc ascending, among the docs of the registered allow-list maskID[q] (-1 / nil: every doc) (ss_vector_topk).
func (s *Scorer) VectorTopK(qvec []int8, maskID []int32, k int) ([][]VecHit, error) {
	if s.vecDim < 1 {
		return nil, fmt.Errorf("VectorTopK: no doc vectors registered (SetDocVectors)")
	}
	nq := len(qvec) / s.vecDim
	if nq == 0 {
		return nil, nil
	}
	kk := k
	if kk < 1 {
		kk = 1
	}
	raw := make([]C.ss_vec_hit, nq*kk)
	nHits := make([]int32, nq)
	rc := C.ss_vector_topk(s.h, C.int32_t(nq), i8p(qvec), i32p(maskID), C.int32_t(k), (*C.ss_vec_hit)(unsafe.Pointer(&raw[0])), i32p(nHits))
	if err := statusErr(s.ctx, rc, "ss_vector_topk"); err != nil {
		return nil, err
	}
	out := make([][]VecHit, nq)
	for q := 0; q < nq; q++ {
		out[q] = make([]VecHit, nHits[q])
		for i := range out[q] {
			r := raw[q*kk+i]
			out[q][i] = VecHit{uint32(r.doc), int32(r.score)}
		}
	}
	return out, nil
}

// SetVectorLists registers a partition of the vector table (ss_scorer_set_vector_lists): centroids[l*dim+i] = position i of list l's
// centroid, listOfDoc[d] = the list of doc d (below nLists) or C.SS_NO_LIST for a doc no probed search finds.  nLists 0 clears.  Needs
// SetDocVectors, which also drops the lists.  The device keeps a second, list-major copy of the table.
func (s *Scorer) SetVectorLists(nLists int, centroids []int8, listOfDoc []uint32) error {
	if nLists > 0 && (s.vecDim < 1 || len(centroids) < nLists*s.vecDim || uint64(len(listOfDoc)) < s.nDocs) {
		return fmt.Errorf("SetVectorLists: %d centroid values and %d docs for %d lists of dim %d over %d docs", len(centroids), len(listOfDoc), nLists, s.vecDim, s.nDocs)
	}
	rc := C.ss_scorer_set_vector_lists(s.h, C.int32_t(nLists), i8p(centroids), u32p(listOfDoc))
	if err := statusErr(s.ctx, rc, "ss_scorer_set_vector_lists"); err != nil {
		return err
	}
	s.nVecLists = nLists
	return nil
}

// AssignVectorLists returns per doc of the vector table the list whose centroid has the largest integer dot product with the doc's
// vector, ties to the lower list, and that score (ss_vector_assign_lists).  It registers nothing.
func (s *Scorer) AssignVectorLists(nLists int, centroids []int8) ([]uint32, []int32, error) {
	if s.vecDim < 1 {
		return nil, nil, fmt.Errorf("AssignVectorLists: no doc vectors registered (SetDocVectors)")
	}
	if nLists < 1 || len(centroids) < nLists*s.vecDim {
		return nil, nil, fmt.Errorf("AssignVectorLists: %d centroid values for %d lists of dim %d", len(centroids), nLists, s.vecDim)
	}
	lists := make([]uint32, s.nDocs)
	scores := make([]int32, s.nDocs)
	rc := C.ss_vector_assign_lists(s.h, C.int32_t(nLists), i8p(centroids), u32p(lists), i32p(scores))
	if err := statusErr(s.ctx, rc, "ss_vector_assign_lists"); err != nil {
		return nil, nil, err
	}
	return lists, scores, nil
}

// VectorTopKProbed is VectorTopK over the docs of the min(nProbe, nLists) lists whose centroids score highest under the query
// (ss_vector_topk_probed): exact within them, and VectorTopK's rows when every list is probed and no doc is at C.SS_NO_LIST.  The
// second result holds each query's probed lists in probe order.
func (s *Scorer) VectorTopKProbed(qvec []int8, maskID []int32, k int, nProbe int) ([][]VecHit, [][]uint32, error) {
	if s.vecDim < 1 {
		return nil, nil, fmt.Errorf("VectorTopKProbed: no doc vectors registered (SetDocVectors)")
	}
	if s.nVecLists < 1 {
		return nil, nil, fmt.Errorf("VectorTopKProbed: no vector lists registered (SetVectorLists)")
	}
	nq := len(qvec) / s.vecDim
	if nq == 0 {
		return nil, nil, nil
	}
	kk := k
	if kk < 1 {
		kk = 1
	}
	np := nProbe
	if np > s.nVecLists {
		np = s.nVecLists
	}
	if np < 1 {
		np = 1
	}
	raw := make([]C.ss_vec_hit, nq*kk)
	nHits := make([]int32, nq)
	probes := make([]uint32, nq*np)
	rc := C.ss_vector_topk_probed(s.h, C.int32_t(nq), i8p(qvec), i32p(maskID), C.int32_t(k), C.int32_t(nProbe),
		(*C.ss_vec_hit)(unsafe.Pointer(&raw[0])), i32p(nHits), u32p(probes))
	if err := statusErr(s.ctx, rc, "ss_vector_topk_probed"); err != nil {
		return nil, nil, err
	}
	out := make([][]VecHit, nq)
	lists := make([][]uint32, nq)
	for q := 0; q < nq; q++ {
		out[q] = make([]VecHit, nHits[q])
		for i := range out[q] {
			r := raw[q*kk+i]
			out[q][i] = VecHit{uint32(r.doc), int32(r.score)}
		}
		lists[q] = probes[q*np : (q+1)*np]
	}
	return out, lists, nil
}

// vecWindow lays hits out as [nq][kIn] ss_hit rows with their counts
func vecWindow(hits [][]Hit) ([]C.ss_hit, []int32, int) {
	nq, kIn := len(hits), 1
	for q := 0; q < nq; q++ {
		if len(hits[q]) > kIn {
			kIn = len(hits[q])
		}
	}
	in := make([]C.ss_hit, nq*kIn)
	nIn := make([]int32, nq)
	for q := 0; q < nq; q++ {
		nIn[q] = int32(len(hits[q]))
		for j, h := range hits[q] {
			in[q*kIn+j] = C.ss_hit{doc: C.uint32_t(h.Doc), title: C.double(h.Title), body: C.double(h.Body), pagerank: C.double(h.PageRank),
				final: C.double(h.Final)}
		}
	}
	return in, nIn, kIn
}

// HitVectorScores returns the score of every hit under its query's vector (ss_hit_vector_scores); C.SS_NO_VEC_SCORE for a doc
// outside the table.
func (s *Scorer) HitVectorScores(qvec []int8, hits [][]Hit) ([][]int32, error) {
	nq := len(hits)
	if nq == 0 {
		return nil, nil
	}
	in, nIn, kIn := vecWindow(hits)
	vals := make([]int32, nq*kIn)
	rc := C.ss_hit_vector_scores(s.h, C.int32_t(nq), i8p(qvec), C.int32_t(kIn), (*C.ss_hit)(unsafe.Pointer(&in[0])), i32p(nIn), i32p(vals))
	if err := statusErr(s.ctx, rc, "ss_hit_vector_scores"); err != nil {
		return nil, err
	}
	out := make([][]int32, nq)
	for q := 0; q < nq; q++ {
		out[q] = append([]int32(nil), vals[q*kIn:q*kIn+len(hits[q])]...)
	}
	return out, nil
}

// RerankHitsByVector sorts every window stably by its rows' scores under the query's vector, descending, rows outside the table
// last, and returns page [first, first+k) with the rows' scores (ss_rerank_hits_by_vector).
func (s *Scorer) RerankHitsByVector(qvec []int8, hits [][]Hit, first, k int) ([][]Hit, [][]int32, error) {
	nq := len(hits)
	if nq == 0 {
		return nil, nil, nil
	}
	in, nIn, kIn := vecWindow(hits)
	kk := k
	if kk < 1 {
		kk = 1
	}
	raw := make([]C.ss_hit, nq*kk)
	nHits, vals := make([]int32, nq), make([]int32, nq*kk)
	rc := C.ss_rerank_hits_by_vector(s.h, C.int32_t(nq), i8p(qvec), C.int32_t(kIn), (*C.ss_hit)(unsafe.Pointer(&in[0])), i32p(nIn),
		C.int32_t(first), C.int32_t(k), (*C.ss_hit)(unsafe.Pointer(&raw[0])), i32p(nHits), i32p(vals))
	if err := statusErr(s.ctx, rc, "ss_rerank_hits_by_vector"); err != nil {
		return nil, nil, err
	}
	out, outVals := make([][]Hit, nq), make([][]int32, nq)
	for q := 0; q < nq; q++ {
		n := int(nHits[q])
		out[q], outVals[q] = make([]Hit, n), append([]int32(nil), vals[q*kk:q*kk+n]...)
		for i := 0; i < n; i++ {
			r := raw[q*kk+i]
			out[q][i] = Hit{uint32(r.doc), float64(r.title), float64(r.body), float64(r.pagerank), float64(r.final)}
		}
	}
	return out, outVals, nil
}

// SetDocTokens registers the token vectors of every doc (ss_scorer_set_doc_tokens): the tokens of doc d are rows tokPtr[d] ..
// tokPtr[d+1] of tok, each of dim int8 values, dim a multiple of 64 up to C.SS_MAX_VEC_DIM.  dim 0 clears.  Independent of
// SetDocVectors.  Register it again after an index update, like the vectors.
func (s *Scorer) SetDocTokens(dim int, tokPtr []uint64, tok []int8) error {
	if dim > 0 && len(tok) > 0 {
		if uint64(len(tokPtr)) != s.nDocs+1 {
			return fmt.Errorf("SetDocTokens: %d pointer entries for %d docs", len(tokPtr), s.nDocs)
		}
		if uint64(len(tok)) < tokPtr[s.nDocs]*uint64(dim) {
			return fmt.Errorf("SetDocTokens: %d values for %d tokens of dim %d", len(tok), tokPtr[s.nDocs], dim)
		}
	}
	rc := C.ss_scorer_set_doc_tokens(s.h, C.int32_t(dim), u64p(tokPtr), i8p(tok))
	return statusErr(s.ctx, rc, "ss_scorer_set_doc_tokens")
}

// maxSimQueries flattens the queries' token vectors: qtPtr[q] .. qtPtr[q+1] are the rows of query q.
func maxSimQueries(qtok [][][]int8) ([]uint32, []int8) {
	qtPtr := make([]uint32, len(qtok)+1)
	var flat []int8
	for q, toks := range qtok {
		for _, v := range toks {
			flat = append(flat, v...)
		}
		qtPtr[q+1] = qtPtr[q] + uint32(len(toks))
	}
	return qtPtr, flat
}

// HitMaxSimScores returns the late-interaction score of every hit under its query's token vectors (ss_hit_maxsim_scores): the
// sum, over the query's tokens, of the best dot product among the doc's tokens; C.SS_NO_VEC_SCORE for a doc outside the table or
// without tokens.  qtok[q]: at most C.SS_MAX_QUERY_TOKENS vectors of the table's dim.
func (s *Scorer) HitMaxSimScores(qtok [][][]int8, hits [][]Hit) ([][]int32, error) {
	nq := len(hits)
	if nq == 0 {
		return nil, nil
	}
	if len(qtok) != nq {
		return nil, fmt.Errorf("HitMaxSimScores: %d queries for %d windows", len(qtok), nq)
	}
	qtPtr, flat := maxSimQueries(qtok)
	in, nIn, kIn := vecWindow(hits)
	vals := make([]int32, nq*kIn)
	rc := C.ss_hit_maxsim_scores(s.h, C.int32_t(nq), u32p(qtPtr), i8p(flat), C.int32_t(kIn), (*C.ss_hit)(unsafe.Pointer(&in[0])), i32p(nIn), i32p(vals))
	if err := statusErr(s.ctx, rc, "ss_hit_maxsim_scores"); err != nil {
		return nil, err
	}
	out := make([][]int32, nq)
	for q := 0; q < nq; q++ {
		out[q] = append([]int32(nil), vals[q*kIn:q*kIn+len(hits[q])]...)
	}
	return out, nil
}

// RerankByMaxSim sorts every window stably by its rows' late-interaction scores under the query's token vectors, descending, rows
// without a score last, and returns page [first, first+k) with the rows' scores (ss_rerank_hits_by_maxsim).
func (s *Scorer) RerankByMaxSim(qtok [][][]int8, hits [][]Hit, first, k int) ([][]Hit, [][]int32, error) {
	nq := len(hits)
	if nq == 0 {
		return nil, nil, nil
	}
	if len(qtok) != nq {
		return nil, nil, fmt.Errorf("RerankByMaxSim: %d queries for %d windows", len(qtok), nq)
	}
	qtPtr, flat := maxSimQueries(qtok)
	in, nIn, kIn := vecWindow(hits)
	kk := k
	if kk < 1 {
		kk = 1
	}
	raw := make([]C.ss_hit, nq*kk)
	nHits, vals := make([]int32, nq), make([]int32, nq*kk)
	rc := C.ss_rerank_hits_by_maxsim(s.h, C.int32_t(nq), u32p(qtPtr), i8p(flat), C.int32_t(kIn), (*C.ss_hit)(unsafe.Pointer(&in[0])), i32p(nIn),
		C.int32_t(first), C.int32_t(k), (*C.ss_hit)(unsafe.Pointer(&raw[0])), i32p(nHits), i32p(vals))
	if err := statusErr(s.ctx, rc, "ss_rerank_hits_by_maxsim"); err != nil {
		return nil, nil, err
	}
	out, outVals := make([][]Hit, nq), make([][]int32, nq)
	for q := 0; q < nq; q++ {
		n := int(nHits[q])
		out[q], outVals[q] = make([]Hit, n), append([]int32(nil), vals[q*kk:q*kk+n]...)
		for i := 0; i < n; i++ {
			r := raw[q*kk+i]
			out[q][i] = Hit{uint32(r.doc), float64(r.title), float64(r.body), float64(r.pagerank), float64(r.final)}
		}
	}
	return out, outVals, nil
}

// MaxSimTopK returns per query the exact k best docs by late-interaction score over every doc that has a token, score descending
// then doc ascending, among the docs of the registered allow-list maskID[q] (-1 / nil: every doc) (ss_maxsim_topk).  qtok[q]: at most
// C.SS_MAX_QUERY_TOKENS vectors of the table's dim; a query without tokens scores every doc 0.
func (s *Scorer) MaxSimTopK(qtok [][][]int8, maskID []int32, k int) ([][]VecHit, error) {
	nq := len(qtok)
	if nq == 0 {
		return nil, nil
	}
	if maskID != nil && len(maskID) != nq {
		return nil, fmt.Errorf("MaxSimTopK: %d mask ids for %d queries", len(maskID), nq)
	}
	qtPtr, flat := maxSimQueries(qtok)
	kk := k
	if kk < 1 {
		kk = 1
	}
	raw := make([]C.ss_vec_hit, nq*kk)
	nHits := make([]int32, nq)
	rc := C.ss_maxsim_topk(s.h, C.int32_t(nq), u32p(qtPtr), i8p(flat), i32p(maskID), C.int32_t(k), (*C.ss_vec_hit)(unsafe.Pointer(&raw[0])), i32p(nHits))
	if err := statusErr(s.ctx, rc, "ss_maxsim_topk"); err != nil {
		return nil, err
	}
	out := make([][]VecHit, nq)
	for q := 0; q < nq; q++ {
		out[q] = make([]VecHit, nHits[q])
		for i := range out[q] {
			r := raw[q*kk+i]
			out[q][i] = VecHit{uint32(r.doc), int32(r.score)}
		}
	}
	return out, nil
}

// DivInfo says why a row of a diversified page was chosen (ss_div_info): its relevance and its largest similarity to the rows chosen
// before it (C.SS_NO_VEC_SCORE for the first row; both C.SS_NO_VEC_SCORE for a doc outside the table).
type DivInfo struct {
	Rel, Sim int32
}

// DiversifyHits re-ranks every window greedily: each next row is the one with the largest wRel*rel - wDiv*(largest similarity of its
// doc vector to a row already chosen), of equal values the earlier row; rows outside the table last; page [first, first+k)
// (ss_diversify_hits).  rel is the row's score under the query's vector, or, with qvec nil, minus its window position.  The weights
// are integers in [0, C.SS_DIV_WEIGHT_MAX].
func (s *Scorer) DiversifyHits(qvec []int8, hits [][]Hit, wRel, wDiv, first, k int) ([][]Hit, [][]DivInfo, error) {
	nq := len(hits)
	if nq == 0 {
		return nil, nil, nil
	}
	in, nIn, kIn := vecWindow(hits)
	kk := k
	if kk < 1 {
		kk = 1
	}
	raw := make([]C.ss_hit, nq*kk)
	nHits, info := make([]int32, nq), make([]C.ss_div_info, nq*kk)
	rc := C.ss_diversify_hits(s.h, C.int32_t(nq), i8p(qvec), C.int32_t(kIn), (*C.ss_hit)(unsafe.Pointer(&in[0])), i32p(nIn),
		C.int32_t(wRel), C.int32_t(wDiv), C.int32_t(first), C.int32_t(k), (*C.ss_hit)(unsafe.Pointer(&raw[0])), i32p(nHits),
		(*C.ss_div_info)(unsafe.Pointer(&info[0])))
	if err := statusErr(s.ctx, rc, "ss_diversify_hits"); err != nil {
		return nil, nil, err
	}
	out, outInfo := make([][]Hit, nq), make([][]DivInfo, nq)
	for q := 0; q < nq; q++ {
		n := int(nHits[q])
		out[q], outInfo[q] = make([]Hit, n), make([]DivInfo, n)
		for i := 0; i < n; i++ {
			r := raw[q*kk+i]
			out[q][i] = Hit{uint32(r.doc), float64(r.title), float64(r.body), float64(r.pagerank), float64(r.final)}
			outInfo[q][i] = DivInfo{int32(info[q*kk+i].rel), int32(info[q*kk+i].sim)}
		}
	}
	return out, outInfo, nil
}

// FuseParams says how FuseHits / HybridTopK merge the two rankings (ss_fuse_params): Mode C.SS_FUSE_RRF (wLex/(RrfC+lexical rank) +
// wVec/(RrfC+vector rank)) or C.SS_FUSE_WEIGHTED (wLex*FinalRank + wVec*vector score).
type FuseParams struct {
	Mode, RrfC int
	WLex, WVec float64
}

// FusedHit is one row of a fused page: the completed lexical row, its fused score, its vector score and its 1-based rank in each
// list (0: the list does not hold the doc).
type FusedHit struct {
	Hit
	Score            float64
	VecScore         int32
	LexRank, VecRank uint16
}

// FusedPage is one page of a query's fused ranking; Union = the distinct docs of both lists.
type FusedPage struct {
	Hits  []FusedHit
	Union int
}

func fusedPages(nq, kk int, raw []C.ss_hit, fused []C.ss_fused, nHits, union []int32) []FusedPage {
	out := make([]FusedPage, nq)
	for q := 0; q < nq; q++ {
		n := int(nHits[q])
		out[q].Union = int(union[q])
		out[q].Hits = make([]FusedHit, n)
		for i := 0; i < n; i++ {
			r, f := raw[q*kk+i], fused[q*kk+i]
			out[q].Hits[i] = FusedHit{Hit{uint32(r.doc), float64(r.title), float64(r.body), float64(r.pagerank), float64(r.final)},
				float64(f.score), int32(f.vec_score), uint16(f.lex_rank), uint16(f.vec_rank)}
		}
	}
	return out
}

// ScoreDocs returns the row that query q's ranking holds for every doc of docs[q], whether or not the doc would reach any top-k
// (ss_score_docs): FinalRank for the output of VectorTopK, SimilarTopK or GraphHitLinks.  A doc outside the tables gives a zero row.
func (s *Scorer) ScoreDocs(qPtr, qTerms []uint32, queryLen []int32, topicProbs []float64, docs [][]uint32) ([][]Hit, error) {
	nq := len(qPtr) - 1
	if nq <= 0 || len(docs) != nq {
		return nil, nil
	}
	kIn := 1
	for q := 0; q < nq; q++ {
		if len(docs[q]) > kIn {
			kIn = len(docs[q])
		}
	}
	in, nIn := make([]uint32, nq*kIn), make([]int32, nq)
	for q := 0; q < nq; q++ {
		nIn[q] = int32(len(docs[q]))
		copy(in[q*kIn:], docs[q])
	}
	raw := make([]C.ss_hit, nq*kIn)
	rc := C.ss_score_docs(s.h, C.int32_t(nq), u32p(qPtr), u32p(qTerms), i32p(queryLen), f64p(topicProbs), C.int32_t(kIn), u32p(in), i32p(nIn),
		(*C.ss_hit)(unsafe.Pointer(&raw[0])))
	if err := statusErr(s.ctx, rc, "ss_score_docs"); err != nil {
		return nil, err
	}
	out := make([][]Hit, nq)
	for q := 0; q < nq; q++ {
		out[q] = make([]Hit, len(docs[q]))
		for i := range out[q] {
			r := raw[q*kIn+i]
			out[q][i] = Hit{uint32(r.doc), float64(r.title), float64(r.body), float64(r.pagerank), float64(r.final)}
		}
	}
	return out, nil
}

// FuseHits merges the lexical list lex[q] and the vector list vec[q] of every query into one ranking by fp and returns page
// [first, first+k) (ss_fuse_hits).  A doc only one list holds is completed on the device: its lexical row as ScoreDocs gives it, its
// vector score as HitVectorScores does; the rows given are trusted.
func (s *Scorer) FuseHits(qPtr, qTerms []uint32, queryLen []int32, topicProbs []float64, qvec []int8, lex [][]Hit, vec [][]VecHit,
	fp FuseParams, first, k int) ([]FusedPage, error) {
	nq := len(qPtr) - 1
	if nq <= 0 || len(lex) != nq || len(vec) != nq {
		return nil, nil
	}
	in, nLex, kLex := vecWindow(lex)
	kVec := 1
	for q := 0; q < nq; q++ {
		if len(vec[q]) > kVec {
			kVec = len(vec[q])
		}
	}
	vin, nVec := make([]C.ss_vec_hit, nq*kVec), make([]int32, nq)
	for q := 0; q < nq; q++ {
		nVec[q] = int32(len(vec[q]))
		for j, v := range vec[q] {
			vin[q*kVec+j] = C.ss_vec_hit{doc: C.uint32_t(v.Doc), score: C.int32_t(v.Score)}
		}
	}
	kk := k
	if kk < 1 {
		kk = 1
	}
	cfp := C.ss_fuse_params{mode: C.int32_t(fp.Mode), rrf_c: C.int32_t(fp.RrfC), w_lex: C.double(fp.WLex), w_vec: C.double(fp.WVec)}
	raw, fused := make([]C.ss_hit, nq*kk), make([]C.ss_fused, nq*kk)
	nHits, union := make([]int32, nq), make([]int32, nq)
	rc := C.ss_fuse_hits(s.h, C.int32_t(nq), u32p(qPtr), u32p(qTerms), i32p(queryLen), f64p(topicProbs), i8p(qvec), C.int32_t(kLex),
		(*C.ss_hit)(unsafe.Pointer(&in[0])), i32p(nLex), C.int32_t(kVec), (*C.ss_vec_hit)(unsafe.Pointer(&vin[0])), i32p(nVec),
		(*C.ss_fuse_params)(unsafe.Pointer(&cfp)), C.int32_t(first), C.int32_t(k), (*C.ss_hit)(unsafe.Pointer(&raw[0])), i32p(nHits),
		(*C.ss_fused)(unsafe.Pointer(&fused[0])), i32p(union))
	if err := statusErr(s.ctx, rc, "ss_fuse_hits"); err != nil {
		return nil, err
	}
	return fusedPages(nq, kk, raw, fused, nHits, union), nil
}

// HybridTopK = ScoreTopKMasked without phrases and VectorTopK, both at k = kWindow under maskID (nil = none), then FuseHits on
// their rows, in one library call: neither window leaves the device (ss_hybrid_topk).
func (s *Scorer) HybridTopK(qPtr, qTerms []uint32, queryLen []int32, topicProbs []float64, qvec []int8, maskID []int32, kWindow int,
	fp FuseParams, first, k int) ([]FusedPage, error) {
	nq := len(qPtr) - 1
	if nq <= 0 {
		return nil, nil
	}
	kk := k
	if kk < 1 {
		kk = 1
	}
	cfp := C.ss_fuse_params{mode: C.int32_t(fp.Mode), rrf_c: C.int32_t(fp.RrfC), w_lex: C.double(fp.WLex), w_vec: C.double(fp.WVec)}
	raw, fused := make([]C.ss_hit, nq*kk), make([]C.ss_fused, nq*kk)
	nHits, union := make([]int32, nq), make([]int32, nq)
	rc := C.ss_hybrid_topk(s.h, C.int32_t(nq), u32p(qPtr), u32p(qTerms), i32p(queryLen), f64p(topicProbs), i8p(qvec), i32p(maskID),
		C.int32_t(kWindow), (*C.ss_fuse_params)(unsafe.Pointer(&cfp)), C.int32_t(first), C.int32_t(k),
		(*C.ss_hit)(unsafe.Pointer(&raw[0])), i32p(nHits), (*C.ss_fused)(unsafe.Pointer(&fused[0])), i32p(union))
	if err := statusErr(s.ctx, rc, "ss_hybrid_topk"); err != nil {
		return nil, err
	}
	return fusedPages(nq, kk, raw, fused, nHits, union), nil
}

// ScoreTopKConstrained = ScoreTopKMasked with query operators: reqPtr/reqTerms name each query's required terms ("+word": every
// result contains it, title or body), excPtr/excTerms its excluded ones ("-word": no result does); nil pointers = none.  The
// constraint terms only filter; put a required word in qTerms too for it to be scored.
func (s *Scorer) ScoreTopKConstrained(qPtr, qTerms, pPtr, pTerms []uint32, queryLen []int32, topicProbs []float64, maskID []int32,
	reqPtr, reqTerms, excPtr, excTerms []uint32, k int) ([][]Hit, error) {
	nq := len(qPtr) - 1
	if nq == 0 {
		return nil, nil
	}
	raw := make([]C.ss_hit, nq*k)
	nHits := make([]int32, nq)
	rc := C.ss_score_topk_constrained(s.h, C.int32_t(nq), u32p(qPtr), u32p(qTerms), u32p(pPtr), u32p(pTerms), i32p(queryLen),
		f64p(topicProbs), i32p(maskID), u32p(reqPtr), u32p(reqTerms), u32p(excPtr), u32p(excTerms), C.int32_t(k),
		(*C.ss_hit)(unsafe.Pointer(&raw[0])), i32p(nHits))
	if err := statusErr(s.ctx, rc, "ss_score_topk_constrained"); err != nil {
		return nil, err
	}
	out := make([][]Hit, nq)
	for q := 0; q < nq; q++ {
		out[q] = make([]Hit, nHits[q])
		for i := range out[q] {
			r := raw[q*k+i]
			out[q][i] = Hit{uint32(r.doc), float64(r.title), float64(r.body), float64(r.pagerank), float64(r.final)}
		}
	}
	return out, nil
}

// ScoreTopKPhrase = ScoreTopK plus one (concatenated) quoted phrase per query (retrieval/phrase.go).
func (s *Scorer) ScoreTopKPhrase(qPtr, qTerms, pPtr, pTerms []uint32, queryLen []int32, topicProbs []float64, k int) ([][]Hit, error) {
	nq := len(qPtr) - 1
	if nq == 0 {
		return nil, nil
	}
	raw := make([]C.ss_hit, nq*k)
	nHits := make([]int32, nq)
	rc := C.ss_score_topk_phrase(s.h, C.int32_t(nq), u32p(qPtr), u32p(qTerms), u32p(pPtr), u32p(pTerms), i32p(queryLen),
		f64p(topicProbs), C.int32_t(k), (*C.ss_hit)(unsafe.Pointer(&raw[0])), i32p(nHits))
	if err := statusErr(s.ctx, rc, "ss_score_topk_phrase"); err != nil {
		return nil, err // the caller decides: a serving path must not die of one bad request
	}
	out := make([][]Hit, nq)
	for q := 0; q < nq; q++ {
		out[q] = make([]Hit, nHits[q])
		for i := range out[q] {
			r := raw[q*k+i]
			out[q][i] = Hit{uint32(r.doc), float64(r.title), float64(r.body), float64(r.pagerank), float64(r.final)}
		}
	}
	return out, nil
}

// ScoreTopK scores a batch of OR queries; safe to call from many goroutines (the library
// serialises calls on one context).  topicProbs may be nil (reference default: sqd = 0).
func (s *Scorer) ScoreTopK(qPtr, qTerms []uint32, queryLen []int32, topicProbs []float64, k int) ([][]Hit, error) {
	nq := len(qPtr) - 1
	raw := make([]C.ss_hit, nq*k)
	nHits := make([]int32, nq)
	rc := C.ss_score_topk(s.h, C.int32_t(nq), u32p(qPtr), u32p(qTerms), i32p(queryLen), f64p(topicProbs), C.int32_t(k),
		(*C.ss_hit)(unsafe.Pointer(&raw[0])), i32p(nHits))
	if err := statusErr(s.ctx, rc, "ss_score_topk"); err != nil {
		return nil, err
	}
	out := make([][]Hit, nq)
	for q := 0; q < nq; q++ {
		out[q] = make([]Hit, nHits[q])
		for i := range out[q] {
			r := raw[q*k+i]
			out[q][i] = Hit{uint32(r.doc), float64(r.title), float64(r.body), float64(r.pagerank), float64(r.final)}
		}
	}
	return out, nil
}

// Ticket names a batch in flight (Submit .. Collect).
type Ticket struct {
	id    C.uint64_t
	nq, k int
}

// ScoreInflight is the number of submitted batches one scorer holds at a time (SS_SCORE_INFLIGHT): a further Submit is refused
// with SS_ERR_STATE until one has been collected.
const ScoreInflight = int(C.SS_SCORE_INFLIGHT)

// Submit enqueues a batch of queries (pPtr / pTerms nil: no quoted phrases) and returns at once; up to C.SS_SCORE_INFLIGHT batches may be in flight.  A server
// goroutine that has the next batch of requests ready calls Submit for it before it Collects the previous one: the host-side
// plan of batch i+1 and the copy-out of batch i-1 then run under the kernels of batch i.
func (s *Scorer) Submit(qPtr, qTerms, pPtr, pTerms []uint32, queryLen []int32, topicProbs []float64, k int) (Ticket, error) {
	nq := len(qPtr) - 1
	var id C.uint64_t
	rc := C.ss_score_topk_submit(s.h, C.int32_t(nq), u32p(qPtr), u32p(qTerms), u32p(pPtr), u32p(pTerms), i32p(queryLen), f64p(topicProbs), C.int32_t(k), &id)
	if err := statusErr(s.ctx, rc, "ss_score_topk_submit"); err != nil {
		return Ticket{}, err
	}
	return Ticket{id, nq, k}, nil
}

// Collect waits for the batch of t and returns its hits like ScoreTopK.
func (s *Scorer) Collect(t Ticket) ([][]Hit, error) {
	raw := make([]C.ss_hit, t.nq*t.k+1)
	nHits := make([]int32, t.nq+1)
	rc := C.ss_score_topk_collect(s.h, t.id, (*C.ss_hit)(unsafe.Pointer(&raw[0])), i32p(nHits))
	if err := statusErr(s.ctx, rc, "ss_score_topk_collect"); err != nil {
		return nil, err
	}
	out := make([][]Hit, t.nq)
	for q := 0; q < t.nq; q++ {
		out[q] = make([]Hit, nHits[q])
		for i := range out[q] {
			r := raw[q*t.k+i]
			out[q][i] = Hit{uint32(r.doc), float64(r.title), float64(r.body), float64(r.pagerank), float64(r.final)}
		}
	}
	return out, nil
}

// MergeHits: multi-GPU doc-range shards only — parts[p] holds shard p's rows of one query batch as returned
// by ScoreTopK (local doc ids), docBase[p] the shard's first corpus doc id.  Returns the k best of the union
// per query in the order of appendSort (util.go:48-54).
func (c *Ctx) MergeHits(parts [][][]Hit, docBase []uint32, k int) [][]Hit {
	np := len(parts)
	nq := len(parts[0])
	raw := make([]C.ss_hit, np*nq*k)
	nHits := make([]int32, np*nq)
	for p := range parts {
		for q := range parts[p] {
			nHits[p*nq+q] = int32(len(parts[p][q]))
			for i, h := range parts[p][q] {
				r := &raw[(p*nq+q)*k+i]
				r.doc, r.title, r.body, r.pagerank, r.final = C.uint32_t(h.Doc), C.double(h.Title), C.double(h.Body), C.double(h.PageRank), C.double(h.Final)
			}
		}
	}
	out := make([]C.ss_hit, nq*k)
	nOut := make([]int32, nq)
	check(c, C.ss_merge_hits(c.h, C.int32_t(nq), C.int32_t(np), C.int32_t(k), (*C.ss_hit)(unsafe.Pointer(&raw[0])), i32p(nHits),
		u32p(docBase), (*C.ss_hit)(unsafe.Pointer(&out[0])), i32p(nOut)), "ss_merge_hits")
	res := make([][]Hit, nq)
	for q := 0; q < nq; q++ {
		res[q] = make([]Hit, nOut[q])
		for i := range res[q] {
			r := out[q*k+i]
			res[q][i] = Hit{uint32(r.doc), float64(r.title), float64(r.body), float64(r.pagerank), float64(r.final)}
		}
	}
	return res
}

// Lexicon is the vocabulary on the device (ss_lexicon): the words of forw[0] keyed by dense term id.  It answers the reference's
// /wordlist/{pre} route (cmd/server/server.go:54-85) a page at a time and suggests known words for a misspelt one.  Immutable apart
// from the frequencies: after an index update that adds terms, Close it and make a new one.
type Lexicon struct {
	h     *C.ss_lexicon
	ctx   *Ctx
	words []string
}

func u8p(s []byte) *C.uint8_t {
	if len(s) == 0 {
		return nil
	}
	return (*C.uint8_t)(unsafe.Pointer(&s[0]))
}

// flattenWords packs words into the (offsets, bytes) pair the library takes.
func flattenWords(words []string) ([]uint32, []byte) {
	ptr := make([]uint32, len(words)+1)
	var data []byte
	for i, w := range words {
		data = append(data, w...)
		ptr[i+1] = uint32(len(data))
	}
	return ptr, data
}

// NewLexicon uploads the words (word t = words[t], any bytes) with their popularity freq (nil = all 0; the retrieval shim passes
// title list length + body list length).
func (c *Ctx) NewLexicon(words []string, freq []uint32) *Lexicon {
	ptr := make([]uint64, len(words)+1)
	var data []byte
	for i, w := range words {
		data = append(data, w...)
		ptr[i+1] = uint64(len(data))
	}
	lx := &Lexicon{ctx: c, words: words}
	check(c, C.ss_lexicon_create(c.h, C.uint64_t(len(words)), u64p(ptr), u8p(data), u32p(freq), &lx.h), "ss_lexicon_create")
	return lx
}

func (lx *Lexicon) Close() { C.ss_lexicon_destroy(lx.h) }

// SetFreq replaces the popularity of every word (nil = all 0) without re-creating the lexicon.
func (lx *Lexicon) SetFreq(freq []uint32) {
	check(lx.ctx, C.ss_lexicon_set_freq(lx.h, u32p(freq)), "ss_lexicon_set_freq")
}

// Order returns the permutation that sorts the words as Go's string < does (equal words by term id).
func (lx *Lexicon) Order() []uint32 {
	var n, b C.uint64_t
	check(lx.ctx, C.ss_lexicon_get_info(lx.h, &n, &b), "ss_lexicon_get_info")
	out := make([]uint32, int(n))
	check(lx.ctx, C.ss_lexicon_read_order(lx.h, u32p(out)), "ss_lexicon_read_order")
	return out
}

// WordList is the route's answer, one page of it: the words that start with pre in sorted order, entries first .. first+k, and
// the number of words with the prefix.
func (lx *Lexicon) WordList(pre string, first int64, k int) ([]string, uint64, error) {
	ptr, data := flattenWords([]string{pre})
	terms := make([]uint32, k)
	nOut := make([]int32, 1)
	nMatch := make([]uint64, 1)
	rc := C.ss_lexicon_prefix(lx.h, C.int32_t(1), u32p(ptr), u8p(data), C.int64_t(first), C.int32_t(k), u32p(terms), i32p(nOut), u64p(nMatch))
	if err := statusErr(lx.ctx, rc, "ss_lexicon_prefix"); err != nil {
		return nil, 0, err
	}
	out := make([]string, nOut[0])
	for i := range out {
		out[i] = lx.words[terms[i]]
	}
	return out, nMatch[0], nil
}

// Suggestion is one known word near a query word: its term id, the word, and the byte edit distance (optimal string alignment:
// insert, delete, substitute, swap of two adjacent bytes).
type Suggestion struct {
	Term uint32
	Word string
	Dist int
}

// Suggest returns per query word up to m known words within maxDist edits whose freq is at least minFreq, ordered by distance,
// then freq descending, then term id.  Distance 0 is included: the caller sees that a word is known.
func (lx *Lexicon) Suggest(words []string, maxDist int, minFreq uint32, m int) ([][]Suggestion, error) {
	nq := len(words)
	if nq == 0 {
		return nil, nil
	}
	ptr, data := flattenWords(words)
	terms := make([]uint32, nq*m)
	dist := make([]int32, nq*m)
	nOut := make([]int32, nq)
	rc := C.ss_lexicon_suggest(lx.h, C.int32_t(nq), u32p(ptr), u8p(data), C.int32_t(maxDist), C.uint32_t(minFreq), C.int32_t(m),
		u32p(terms), i32p(dist), i32p(nOut))
	if err := statusErr(lx.ctx, rc, "ss_lexicon_suggest"); err != nil {
		return nil, err
	}
	out := make([][]Suggestion, nq)
	for q := 0; q < nq; q++ {
		out[q] = make([]Suggestion, nOut[q])
		for i := range out[q] {
			t := terms[q*m+i]
			out[q][i] = Suggestion{t, lx.words[t], int(dist[q*m+i])}
		}
	}
	return out, nil
}

// Completion is one word that starts with a typed prefix: its term id, the word and its freq.
type Completion struct {
	Term uint32
	Word string
	Freq uint32
}

// Complete returns per prefix up to m words that start with it and whose freq is at least minFreq, ordered by freq descending, then
// as Go's string < orders the words, then term id (ss_lexicon_complete), and the number of words with the prefix whatever their
// freq.  Written against the header like the rest of this file, not compiled (see the note at the top).
func (lx *Lexicon) Complete(prefixes []string, minFreq uint32, m int) ([][]Completion, []uint64, error) {
	nq := len(prefixes)
	if nq == 0 {
		return nil, nil, nil
	}
	ptr, data := flattenWords(prefixes)
	terms := make([]uint32, nq*m)
	freq := make([]uint32, nq*m)
	nOut := make([]int32, nq)
	nMatch := make([]uint64, nq)
	rc := C.ss_lexicon_complete(lx.h, C.int32_t(nq), u32p(ptr), u8p(data), C.uint32_t(minFreq), C.int32_t(m), u32p(terms), u32p(freq),
		i32p(nOut), u64p(nMatch))
	if err := statusErr(lx.ctx, rc, "ss_lexicon_complete"); err != nil {
		return nil, nil, err
	}
	out := make([][]Completion, nq)
	for q := 0; q < nq; q++ {
		out[q] = make([]Completion, nOut[q])
		for i := range out[q] {
			t := terms[q*m+i]
			out[q][i] = Completion{t, lx.words[t], freq[q*m+i]}
		}
	}
	return out, nMatch, nil
}
