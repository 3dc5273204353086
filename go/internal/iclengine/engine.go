// Package iclengine owns the ONE libimageclust_hip.so context the drop-in packages share (internal/embeddings holds the
// model in it, internal/clustering clusters on it): a process that loads both packages creates one GPU context and one
// set of workspaces, not two.  NOT COMPILED in the authoring container (no Go toolchain): logic-free glue.
package iclengine

/*
#cgo CFLAGS: -I${SRCDIR}/../../../include
#cgo LDFLAGS: -L${SRCDIR}/../../../imageclust_amd -limageclust_hip
#include <stdlib.h>
#include "imageclust.h"
*/
import "C"

import (
	"fmt"
	"os"
	"runtime"
	"strconv"
	"sync"
	"unsafe"
)

var (
	once sync.Once
	ctx  *C.icl_ctx
	err  error
)

// Ctx returns the shared context as an unsafe.Pointer (cgo types are package-local: each caller casts it back to its
// own *C.icl_ctx), creating it on first use.  ICL_DEVICE in the environment selects the GPU (icl_create's device ordinal 0 otherwise).
func Ctx() (unsafe.Pointer, error) {
	once.Do(func() {
		// icl_last_error(NULL) reads a thread-local string: keep the failing call and the read on one OS thread
		runtime.LockOSThread()
		defer runtime.UnlockOSThread()
		dev := 0
		if v, e := strconv.Atoi(os.Getenv("ICL_DEVICE")); e == nil && v >= 0 {
			dev = v
		}
		if rc := C.icl_create(C.int(dev), &ctx); rc != C.ICL_OK {
			err = fmt.Errorf("icl_create: %s", C.GoString(C.icl_last_error(nil)))
		}
	})
	return unsafe.Pointer(ctx), err
}

var (
	modelMu     sync.Mutex
	modelLoaded string // path of the ONNX file whose weights the shared context holds ("" = none)
)

// LoadModelOnce loads the ONNX file into the shared context unless that very file is already loaded: the reference calls
// LoadPretrainedModelONNX once per request (workflow.go), and reloading would stall every embedder in flight behind the context's mutex.
func LoadModelOnce(path string) error {
	raw, e := Ctx()
	if e != nil {
		return e
	}
	modelMu.Lock()
	defer modelMu.Unlock()
	if modelLoaded == path {
		return nil
	}
	p := C.CString(path)
	defer C.free(unsafe.Pointer(p))
	if rc := C.icl_model_load_onnx((*C.icl_ctx)(raw), p); rc != C.ICL_OK {
		return fmt.Errorf("%s", C.GoString(C.icl_last_error((*C.icl_ctx)(raw))))
	}
	modelLoaded = path
	return nil
}

// LastError returns the message of the last failed call on the context (stored in the context, not in TLS).
func LastError() string {
	if ctx == nil {
		return "no context"
	}
	return C.GoString(C.icl_last_error(ctx))
}

// Mid-size route of icl_cluster_many (problems of 257 to 2048 rows, one workgroup each): icl_set_many_options' modes.
const (
	ManyMidAuto = int(C.ICL_MANY_MID_AUTO)
	ManyMidOff  = int(C.ICL_MANY_MID_OFF)
	ManyMidOn   = int(C.ICL_MANY_MID_ON)
)

// SetManyOptions chooses when PerformClusteringWithConstraintsBatch's mid-size problems take that route (same results in every mode).
func SetManyOptions(midMode int) error {
	raw, e := Ctx()
	if e != nil {
		return e
	}
	if rc := C.icl_set_many_options((*C.icl_ctx)(raw), C.int(midMode)); rc != C.ICL_OK {
		return fmt.Errorf("%s", C.GoString(C.icl_last_error((*C.icl_ctx)(raw))))
	}
	return nil
}

// LastManyStats reports the problems of the last icl_cluster_many call by route, and the groups its mid-size problems ran in.
func LastManyStats() (small, mid, large, midGroups int64, err error) {
	raw, e := Ctx()
	if e != nil {
		return 0, 0, 0, 0, e
	}
	var a, b, c, d C.int64_t
	if rc := C.icl_last_many_stats((*C.icl_ctx)(raw), &a, &b, &c, &d); rc != C.ICL_OK {
		return 0, 0, 0, 0, fmt.Errorf("%s", C.GoString(C.icl_last_error((*C.icl_ctx)(raw))))
	}
	return int64(a), int64(b), int64(c), int64(d), nil
}

// SeededProblem is one problem of ClusterManySeeded: Centroids[i] and Sizes[i] describe seed cluster i (a negative size: a frozen
// cluster of that many items, never merged); KTarget > 0 is the number of clusters to stop at, else CalculateOptimalClusters of the item
// total decides.
type SeededProblem struct {
	Centroids        [][]float32
	Sizes            []int32
	MinSize, MaxSize int
	KTarget          int
}

// SeededResult is what icl_cluster_many_seeded gives for one problem, at seed granularity: ClusterID[i] (-1: seed i's cluster is below
// MinSize), SeedRank[i] (its place in the cluster's seed sequence), the merge log as pairs of creation ids (seed i is i, merge t is
// m + t), and COut: the row of each final cluster's rank-0 seed holds that cluster's centroid, every other row is zero.
type SeededResult struct {
	ClusterID, SeedRank []int32
	NClusters           int
	Merges              [][2]int32
	COut                [][]float32
	Status              int // ICL_OK, ICL_ERR_CONSTRAINT (the reference's (nil,false)), ICL_ERR_UNSUPPORTED
}

// ClusterManySeeded resumes the clustering loop (clustering.go:216-246) from existing clusters for many problems in one
// icl_cluster_many_seeded call.  The error is the call's own (a bad argument, the device); a problem's failure is its Status.
func ClusterManySeeded(probs []SeededProblem) ([]SeededResult, error) {
	return clusterManySeeded(probs, nil)
}

// ApartProblem is one problem of ClusterManyApart: a SeededProblem with keep-apart constraints.  ApartClass (nil: none) holds one
// int per seed, 0 meaning none: two different seeds of one non-zero class never share a cluster.  ApartPairs lists seed indices that
// never share a cluster, either order.  A merged cluster inherits the bans of both parents.
type ApartProblem struct {
	SeededProblem
	ApartClass []int32
	ApartPairs [][2]int32
}

// ClusterManyApart is ClusterManySeeded with keep-apart constraints (icl_cluster_many_apart).  The loop may end before KTarget
// clusters are reached: len(Merges) then tells.  A malformed constraint is the call's error; more than ManySeededMax seeds is the
// problem's Status (ICL_ERR_UNSUPPORTED).
func ClusterManyApart(probs []ApartProblem) ([]SeededResult, error) {
	seeded := make([]SeededProblem, len(probs))
	for j, pr := range probs {
		if pr.ApartClass != nil && len(pr.ApartClass) != len(pr.Sizes) {
			return nil, fmt.Errorf("problem %d: %d classes for %d seeds", j, len(pr.ApartClass), len(pr.Sizes))
		}
		seeded[j] = pr.SeededProblem
	}
	return clusterManySeeded(seeded, probs)
}

// the body of both: apart is nil (icl_cluster_many_seeded) or holds every problem's constraints (icl_cluster_many_apart)
func clusterManySeeded(probs []SeededProblem, apart []ApartProblem) ([]SeededResult, error) {
	out := make([]SeededResult, len(probs))
	if len(probs) == 0 {
		return out, nil
	}
	raw, e := Ctx()
	if e != nil {
		return nil, e
	}
	np := len(probs)
	eoff := make([]int64, np)
	m := make([]int32, np)
	d := make([]int32, np)
	mn := make([]int32, np)
	mx := make([]int32, np)
	kt := make([]int32, np)
	total, rows := 0, 0
	for j, pr := range probs {
		if len(pr.Sizes) != len(pr.Centroids) {
			return nil, fmt.Errorf("problem %d: %d sizes for %d centroids", j, len(pr.Sizes), len(pr.Centroids))
		}
		m[j] = int32(len(pr.Centroids))
		if m[j] > 0 {
			d[j] = int32(len(pr.Centroids[0]))
		}
		mn[j], mx[j], kt[j] = int32(pr.MinSize), int32(pr.MaxSize), int32(pr.KTarget)
		eoff[j] = int64(total)
		total += (int(m[j])*int(d[j]) + 3) / 4 * 4 // each problem on a 16-byte boundary
		rows += int(m[j])
	}
	flat := make([]float32, total+1) // [][]float32 cannot cross cgo: one contiguous buffer
	cout := make([]float32, total+1)
	ss := make([]int32, rows+1)
	at := 0
	for j, pr := range probs {
		for i, row := range pr.Centroids {
			copy(flat[int(eoff[j])+i*int(d[j]):], row)
		}
		copy(ss[at:], pr.Sizes)
		at += int(m[j])
	}
	cid := make([]int32, rows+1)
	rank := make([]int32, rows+1)
	mg := make([]int32, 2*rows+1)
	nc := make([]int32, np)
	nm := make([]int32, np)
	st := make([]int32, np)
	for j := range st {
		st[j] = -1 // stays -1 when the call fails before the problems run
	}
	i32 := func(p *int32) *C.int32_t { return (*C.int32_t)(unsafe.Pointer(p)) }
	var rc C.int
	if apart == nil {
		rc = C.icl_cluster_many_seeded((*C.icl_ctx)(raw), C.int32_t(np), (*C.float)(unsafe.Pointer(&flat[0])), C.int64_t(len(flat)),
			(*C.int64_t)(unsafe.Pointer(&eoff[0])), i32(&m[0]), i32(&d[0]), i32(&ss[0]), i32(&mn[0]), i32(&mx[0]), i32(&kt[0]), i32(&cid[0]),
			i32(&rank[0]), i32(&nc[0]), i32(&nm[0]), i32(&mg[0]), i32(&st[0]), (*C.float)(unsafe.Pointer(&cout[0])))
	} else {
		cls := make([]int32, rows+1) // the seed layout of ss; 0: no class
		poff := make([]int64, np+1)
		pairs := []int32{}
		at = 0
		for j, pr := range apart {
			copy(cls[at:], pr.ApartClass)
			at += int(m[j])
			for _, q := range pr.ApartPairs {
				pairs = append(pairs, q[0], q[1])
			}
			poff[j+1] = int64(len(pairs) / 2)
		}
		pairs = append(pairs, 0) // (never empty: its address is taken)
		rc = C.icl_cluster_many_apart((*C.icl_ctx)(raw), C.int32_t(np), (*C.float)(unsafe.Pointer(&flat[0])), C.int64_t(len(flat)),
			(*C.int64_t)(unsafe.Pointer(&eoff[0])), i32(&m[0]), i32(&d[0]), i32(&ss[0]), i32(&mn[0]), i32(&mx[0]), i32(&kt[0]), i32(&cls[0]),
			(*C.int64_t)(unsafe.Pointer(&poff[0])), i32(&pairs[0]), i32(&cid[0]), i32(&rank[0]), i32(&nc[0]), i32(&nm[0]), i32(&mg[0]),
			i32(&st[0]), (*C.float)(unsafe.Pointer(&cout[0])))
	}
	for j := range st {
		if rc != C.ICL_OK && st[j] < 0 {
			return nil, fmt.Errorf("%s", C.GoString(C.icl_last_error((*C.icl_ctx)(raw))))
		}
	}
	at = 0
	for j := range probs {
		r := SeededResult{Status: int(st[j]), NClusters: int(nc[j])}
		r.ClusterID = append([]int32(nil), cid[at:at+int(m[j])]...)
		r.SeedRank = append([]int32(nil), rank[at:at+int(m[j])]...)
		for t := 0; t < int(nm[j]); t++ {
			r.Merges = append(r.Merges, [2]int32{mg[2*at+2*t], mg[2*at+2*t+1]})
		}
		r.COut = make([][]float32, m[j])
		for i := range r.COut {
			o := int(eoff[j]) + i*int(d[j])
			r.COut[i] = append([]float32(nil), cout[o:o+int(d[j])]...)
		}
		out[j] = r
		at += int(m[j])
	}
	return out, nil
}

// ManySeededMax is the cap of icl_cluster_many_seeded and icl_cluster_many_apart on the seeds of one problem; ClusterSeeded and
// ClusterApart have none.
const ManySeededMax = 2048

// ClusterSeeded runs ONE seeded problem on the large-N engine (icl_cluster_seeded: the exact pipeline of ward.hip, any number of seeds).
// The result is ClusterManySeeded's for the same problem, bit for bit; the merge log comes from icl_last_merges.  The error is the call's
// own; ICL_ERR_CONSTRAINT and ICL_ERR_UNSUPPORTED are the result's Status.
func ClusterSeeded(pr SeededProblem) (SeededResult, error) {
	return clusterSeeded(pr, nil, false)
}

// ClusterSeededFast runs the same problem in FAST mode (icl_cluster_seeded_fast: the matrix-core distance matrix scaled by the seeds'
// item counts, Lance-Williams rows; any number of seeds).  Defined by its own restatement, not bit-comparable with ClusterSeeded; a run
// cut and resumed is not the uncut run.  COut is MergeClusters' centroid along the call's own merge log.  No constrained form exists.
func ClusterSeededFast(pr SeededProblem) (SeededResult, error) {
	return clusterSeeded(pr, nil, true)
}

// ClusterApart runs ONE constrained seeded problem on the large-N engine (icl_cluster_apart: the one-merge-per-step exact loop of
// ward.hip under a keep-apart relation, any number of seeds).  The result is ClusterManyApart's for the same problem, bit for bit, and
// with no constraint ClusterSeeded's.  A malformed constraint is the call's error.
func ClusterApart(pr ApartProblem) (SeededResult, error) {
	if pr.ApartClass != nil && len(pr.ApartClass) != len(pr.Sizes) {
		return SeededResult{}, fmt.Errorf("%d classes for %d seeds", len(pr.ApartClass), len(pr.Sizes))
	}
	return clusterSeeded(pr.SeededProblem, &pr, false)
}

// the body of the three: apart is nil (icl_cluster_seeded; icl_cluster_seeded_fast with fast) or holds the problem's constraints
// (icl_cluster_apart, never with fast)
func clusterSeeded(pr SeededProblem, apart *ApartProblem, fast bool) (SeededResult, error) {
	raw, e := Ctx()
	if e != nil {
		return SeededResult{}, e
	}
	if len(pr.Sizes) != len(pr.Centroids) {
		return SeededResult{}, fmt.Errorf("%d sizes for %d centroids", len(pr.Sizes), len(pr.Centroids))
	}
	m, d := len(pr.Centroids), 0
	if m > 0 {
		d = len(pr.Centroids[0])
	}
	flat := make([]float32, m*d+1) // [][]float32 cannot cross cgo: one contiguous buffer
	cout := make([]float32, m*d+1)
	for i, row := range pr.Centroids {
		copy(flat[i*d:], row)
	}
	ss := append(append([]int32(nil), pr.Sizes...), 0)
	cid := make([]int32, m+1)
	rank := make([]int32, m+1)
	var nc C.int32_t
	i32 := func(p *int32) *C.int32_t { return (*C.int32_t)(unsafe.Pointer(p)) }
	var rc C.int
	if apart == nil && fast {
		rc = C.icl_cluster_seeded_fast((*C.icl_ctx)(raw), (*C.float)(unsafe.Pointer(&flat[0])), C.int64_t(m), C.int32_t(d), i32(&ss[0]),
			C.int32_t(pr.MinSize), C.int32_t(pr.MaxSize), C.int32_t(pr.KTarget), i32(&cid[0]), i32(&rank[0]), &nc,
			(*C.float)(unsafe.Pointer(&cout[0])))
	} else if apart == nil {
		rc = C.icl_cluster_seeded((*C.icl_ctx)(raw), (*C.float)(unsafe.Pointer(&flat[0])), C.int64_t(m), C.int32_t(d), i32(&ss[0]),
			C.int32_t(pr.MinSize), C.int32_t(pr.MaxSize), C.int32_t(pr.KTarget), i32(&cid[0]), i32(&rank[0]), &nc,
			(*C.float)(unsafe.Pointer(&cout[0])))
	} else {
		cls := make([]int32, m+1) // 0: no class
		copy(cls, apart.ApartClass)
		pairs := make([]int32, 0, 2*len(apart.ApartPairs)+1)
		for _, q := range apart.ApartPairs {
			pairs = append(pairs, q[0], q[1])
		}
		npairs := len(pairs) / 2
		pairs = append(pairs, 0) // (never empty: its address is taken)
		rc = C.icl_cluster_apart((*C.icl_ctx)(raw), (*C.float)(unsafe.Pointer(&flat[0])), C.int64_t(m), C.int32_t(d), i32(&ss[0]),
			C.int32_t(pr.MinSize), C.int32_t(pr.MaxSize), C.int32_t(pr.KTarget), i32(&cls[0]), C.int64_t(npairs), i32(&pairs[0]),
			i32(&cid[0]), i32(&rank[0]), &nc, (*C.float)(unsafe.Pointer(&cout[0])))
	}
	if rc != C.ICL_OK && rc != C.ICL_ERR_CONSTRAINT && rc != C.ICL_ERR_UNSUPPORTED {
		return SeededResult{}, fmt.Errorf("%s", C.GoString(C.icl_last_error((*C.icl_ctx)(raw))))
	}
	r := SeededResult{Status: int(rc), NClusters: int(nc), ClusterID: cid[:m], SeedRank: rank[:m]}
	if rc == C.ICL_OK {
		nm := int(C.icl_last_merges((*C.icl_ctx)(raw), nil, 0))
		mg := make([]int32, 2*nm+1)
		C.icl_last_merges((*C.icl_ctx)(raw), i32(&mg[0]), C.int64_t(nm))
		for t := 0; t < nm; t++ {
			r.Merges = append(r.Merges, [2]int32{mg[2*t], mg[2*t+1]})
		}
	}
	r.COut = make([][]float32, m)
	for i := range r.COut {
		r.COut[i] = append([]float32(nil), cout[i*d:(i+1)*d]...)
	}
	return r, nil
}

// Nearest is icl_nearest: for each query cluster (queries[i], qSizes[i] items; nil sizes: all 1) the k library clusters (library[j],
// eSizes[j]) of smallest WardDistance, the reference's values bit for bit, ascending by (value, j), NaN last.  exclude (nil: none)
// names a column per query that is skipped (-1: none; a self-join passes i); maxSize > 0 leaves out the pairs whose sizes add up to
// more.  idx and val hold k entries per query; a short row ends in idx -1, val MaxFloat32.  No distance matrix is built.
func Nearest(queries [][]float32, qSizes []int32, library [][]float32, eSizes []int32, k, maxSize int, exclude []int64) (idx [][]int32, val [][]float32, err error) {
	raw, e := Ctx()
	if e != nil {
		return nil, nil, e
	}
	nq, n, d := len(queries), len(library), 0
	if nq > 0 {
		d = len(queries[0])
	} else if n > 0 {
		d = len(library[0])
	}
	if (qSizes != nil && len(qSizes) != nq) || (eSizes != nil && len(eSizes) != n) || (exclude != nil && len(exclude) != nq) {
		return nil, nil, fmt.Errorf("sizes or exclude do not match %d queries and %d library rows", nq, n)
	}
	if k < 1 {
		return nil, nil, fmt.Errorf("k must be 1 .. 64, got %d", k)
	}
	flatQ := make([]float32, nq*d+1) // [][]float32 cannot cross cgo: one contiguous buffer each
	flatE := make([]float32, n*d+1)
	for i, row := range queries {
		copy(flatQ[i*d:(i+1)*d], row)
	}
	for j, row := range library {
		copy(flatE[j*d:(j+1)*d], row)
	}
	fi := make([]int32, nq*k+1)
	fv := make([]float32, nq*k+1)
	i32 := func(s []int32) *C.int32_t {
		if len(s) == 0 {
			return nil
		}
		return (*C.int32_t)(unsafe.Pointer(&s[0]))
	}
	var ex *C.int64_t
	if len(exclude) > 0 {
		ex = (*C.int64_t)(unsafe.Pointer(&exclude[0]))
	}
	if rc := C.icl_nearest((*C.icl_ctx)(raw), (*C.float)(unsafe.Pointer(&flatQ[0])), i32(qSizes), C.int64_t(nq),
		(*C.float)(unsafe.Pointer(&flatE[0])), i32(eSizes), C.int64_t(n), C.int32_t(d), C.int32_t(k), C.int32_t(maxSize), ex,
		(*C.int32_t)(unsafe.Pointer(&fi[0])), (*C.float)(unsafe.Pointer(&fv[0]))); rc != C.ICL_OK {
		return nil, nil, fmt.Errorf("%s", C.GoString(C.icl_last_error((*C.icl_ctx)(raw))))
	}
	idx, val = make([][]int32, nq), make([][]float32, nq)
	for i := range idx {
		idx[i] = fi[i*k : (i+1)*k : (i+1)*k]
		val[i] = fv[i*k : (i+1)*k : (i+1)*k]
	}
	return idx, val, nil
}

// FitResult is what ClusterFit returns: per row its cost against its own cluster and its AltIdx / AltVal alternatives (kAlt entries
// each; a short row ends in -1, MaxFloat32), per cluster the number of rows that name it, the row of smallest own cost and the row
// of largest (-1: nobody names the cluster).
type FitResult struct {
	Own                []float32
	AltIdx             [][]int32
	AltVal             [][]float32
	Listed, Rep, Worst []int32
}

// flatRows copies rows of d floats into one contiguous buffer ([][]float32 cannot cross cgo), one spare entry behind them.
func flatRows(rows [][]float32, d int) []float32 {
	flat := make([]float32, len(rows)*d+1)
	for i, row := range rows {
		copy(flat[i*d:(i+1)*d], row)
	}
	return flat
}

// ClusterFit is icl_cluster_fit: for each clustered row (rows[i], qSizes[i] items; nil sizes: all 1) the WardDistance to its own
// cluster clusterOf[i] of (centroids, cSizes) -- -1: none, cost MaxFloat32 -- and its kAlt (0 .. 64) nearest other clusters, the
// reference's values bit for bit throughout.  A negative cSizes entry is a frozen cluster: measured as an own cluster, never offered;
// maxSize > 0 leaves out the pairs whose sizes add up to more.  No distance matrix is built.
func ClusterFit(rows [][]float32, qSizes []int32, clusterOf []int32, centroids [][]float32, cSizes []int32, kAlt, maxSize int) (FitResult, error) {
	raw, e := Ctx()
	if e != nil {
		return FitResult{}, e
	}
	nq, K, d := len(rows), len(centroids), 0
	if nq > 0 {
		d = len(rows[0])
	} else if K > 0 {
		d = len(centroids[0])
	}
	if (qSizes != nil && len(qSizes) != nq) || (cSizes != nil && len(cSizes) != K) || len(clusterOf) != nq {
		return FitResult{}, fmt.Errorf("sizes or clusterOf do not match %d rows and %d clusters", nq, K)
	}
	if kAlt < 0 {
		return FitResult{}, fmt.Errorf("kAlt must be 0 .. 64, got %d", kAlt)
	}
	flatQ, flatC := flatRows(rows, d), flatRows(centroids, d)
	own := make([]float32, nq+1)
	fi := make([]int32, nq*kAlt+1)
	fv := make([]float32, nq*kAlt+1)
	listed, rep, worst := make([]int32, K+1), make([]int32, K+1), make([]int32, K+1)
	i32 := func(s []int32) *C.int32_t {
		if len(s) == 0 {
			return nil
		}
		return (*C.int32_t)(unsafe.Pointer(&s[0]))
	}
	f32 := func(s []float32) *C.float { return (*C.float)(unsafe.Pointer(&s[0])) }
	if rc := C.icl_cluster_fit((*C.icl_ctx)(raw), f32(flatQ), i32(qSizes), i32(clusterOf), C.int64_t(nq), f32(flatC), i32(cSizes), C.int64_t(K),
		C.int32_t(d), C.int32_t(kAlt), C.int32_t(maxSize), f32(own), i32(fi), f32(fv), i32(listed), i32(rep), i32(worst)); rc != C.ICL_OK {
		return FitResult{}, fmt.Errorf("%s", C.GoString(C.icl_last_error((*C.icl_ctx)(raw))))
	}
	r := FitResult{Own: own[:nq], AltIdx: make([][]int32, nq), AltVal: make([][]float32, nq), Listed: listed[:K], Rep: rep[:K], Worst: worst[:K]}
	for i := range r.AltIdx {
		r.AltIdx[i] = fi[i*kAlt : (i+1)*kAlt : (i+1)*kAlt]
		r.AltVal[i] = fv[i*kAlt : (i+1)*kAlt : (i+1)*kAlt]
	}
	return r, nil
}

// FoldCentroids gives each cluster listed by its members the centroid the reference holds after merging them one at a time in list
// order (icl_fold_centroids: MergeClusters of clustering.go:29-47 folded, bit for bit).  groups[g] lists rows of `rows`; sizes[i] is
// row i's item count (nil: all 1).  Returns one centroid and one item total per group; an empty group gives zeros and 0.
func FoldCentroids(rows [][]float32, sizes []int32, groups [][]int32) ([][]float32, []int32, error) {
	raw, e := Ctx()
	if e != nil {
		return nil, nil, e
	}
	n, K, d := len(rows), len(groups), 0
	if n > 0 {
		d = len(rows[0])
	}
	if sizes != nil && len(sizes) != n {
		return nil, nil, fmt.Errorf("%d sizes for %d rows", len(sizes), n)
	}
	if K == 0 {
		return nil, nil, nil
	}
	if d == 0 {
		return nil, nil, fmt.Errorf("no rows to fold")
	}
	rowPtr := make([]int64, K+1)
	member := make([]int32, 0, n)
	for g, list := range groups {
		member = append(member, list...)
		rowPtr[g+1] = int64(len(member))
	}
	flat := flatRows(rows, d)
	out := make([]float32, K*d)
	total := make([]int32, K)
	i32 := func(s []int32) *C.int32_t {
		if len(s) == 0 {
			return nil
		}
		return (*C.int32_t)(unsafe.Pointer(&s[0]))
	}
	if rc := C.icl_fold_centroids((*C.icl_ctx)(raw), (*C.float)(unsafe.Pointer(&flat[0])), i32(sizes), C.int64_t(n), C.int32_t(d),
		(*C.int64_t)(unsafe.Pointer(&rowPtr[0])), i32(member), C.int64_t(K), (*C.float)(unsafe.Pointer(&out[0])), i32(total)); rc != C.ICL_OK {
		return nil, nil, fmt.Errorf("%s", C.GoString(C.icl_last_error((*C.icl_ctx)(raw))))
	}
	cen := make([][]float32, K)
	for g := range cen {
		cen[g] = out[g*d : (g+1)*d]
	}
	return cen, total, nil
}

// WardValuesAt is icl_ward_values_at: the exact WardDistance of each listed pair (row qi[p] of rows with qSizes, row ej[p] of library
// with eSizes; nil sizes: all 1, a negative eSizes entry a frozen cluster's item count), the reference's values bit for bit.
func WardValuesAt(rows [][]float32, qSizes []int32, library [][]float32, eSizes []int32, qi, ej []int32) ([]float32, error) {
	raw, e := Ctx()
	if e != nil {
		return nil, e
	}
	nq, n, np, d := len(rows), len(library), len(qi), 0
	if nq > 0 {
		d = len(rows[0])
	}
	if (qSizes != nil && len(qSizes) != nq) || (eSizes != nil && len(eSizes) != n) || len(ej) != np {
		return nil, fmt.Errorf("sizes or pair lists do not match %d rows, %d library rows and %d pairs", nq, n, np)
	}
	if np == 0 {
		return nil, nil
	}
	flatQ, flatE := flatRows(rows, d), flatRows(library, d)
	val := make([]float32, np)
	i32 := func(s []int32) *C.int32_t {
		if len(s) == 0 {
			return nil
		}
		return (*C.int32_t)(unsafe.Pointer(&s[0]))
	}
	if rc := C.icl_ward_values_at((*C.icl_ctx)(raw), (*C.float)(unsafe.Pointer(&flatQ[0])), i32(qSizes), C.int64_t(nq),
		(*C.float)(unsafe.Pointer(&flatE[0])), i32(eSizes), C.int64_t(n), C.int32_t(d), i32(qi), i32(ej), C.int64_t(np),
		(*C.float)(unsafe.Pointer(&val[0]))); rc != C.ICL_OK {
		return nil, fmt.Errorf("%s", C.GoString(C.icl_last_error((*C.icl_ctx)(raw))))
	}
	return val, nil
}

// PairsWithin is icl_pairs_within: EVERY pair of rows whose WardDistance (sizes[i] items per row; nil: all 1) is at most threshold, the
// reference's values bit for bit, as a CSR list over the strict lower triangle: col[rowPtr[i]:rowPtr[i+1]] are row i's partners j < i
// in ascending j, val their values.  No cap on a row's partners and no distance matrix.  The size query and the call proper are both
// made here.
func PairsWithin(rows [][]float32, sizes []int32, threshold float32) (rowPtr []int64, col []int32, val []float32, err error) {
	raw, e := Ctx()
	if e != nil {
		return nil, nil, nil, e
	}
	n, d := len(rows), 0
	if n > 0 {
		d = len(rows[0])
	}
	if sizes != nil && len(sizes) != n {
		return nil, nil, nil, fmt.Errorf("%d sizes for %d rows", len(sizes), n)
	}
	if n == 0 { // no rows, no row length to pass: the empty list, as the Python mirror returns it
		return []int64{0}, nil, nil, nil
	}
	flat := make([]float32, n*d+1) // [][]float32 cannot cross cgo: one contiguous buffer
	for i, row := range rows {
		copy(flat[i*d:(i+1)*d], row)
	}
	var sz *C.int32_t
	if len(sizes) > 0 {
		sz = (*C.int32_t)(unsafe.Pointer(&sizes[0]))
	}
	rowPtr = make([]int64, n+1)
	total := C.int64_t(-1)
	call := func(c *C.int32_t, v *C.float, cap int64) C.int {
		return C.icl_pairs_within((*C.icl_ctx)(raw), (*C.float)(unsafe.Pointer(&flat[0])), sz, C.int64_t(n), C.int32_t(d), C.float(threshold),
			(*C.int64_t)(unsafe.Pointer(&rowPtr[0])), c, v, C.int64_t(cap), &total)
	}
	if rc := call(nil, nil, 0); rc != C.ICL_OK {
		return nil, nil, nil, fmt.Errorf("%s", C.GoString(C.icl_last_error((*C.icl_ctx)(raw))))
	}
	t := int64(total)
	col, val = make([]int32, t+1), make([]float32, t+1)
	if t > 0 {
		if rc := call((*C.int32_t)(unsafe.Pointer(&col[0])), (*C.float)(unsafe.Pointer(&val[0])), t); rc != C.ICL_OK {
			return nil, nil, nil, fmt.Errorf("%s", C.GoString(C.icl_last_error((*C.icl_ctx)(raw))))
		}
	}
	return rowPtr, col[:t], val[:t], nil
}

// PairsBetween is icl_pairs_between: EVERY pair (row i of rows, row j of library) whose WardDistance (qSizes[i] and lSizes[j] items; nil:
// all 1) is at most threshold, Nearest's values bit for bit, as a CSR list over the rows: col[rowPtr[i]:rowPtr[i+1]] are row i's library
// partners in ascending j, val their values.  exclude[i] (nil: none; -1: none) is left out of row i: rows that are library rows pass
// their own index.  No cap on a row's partners, no max-size ban and no distance matrix.  The size query and the call proper are both
// made here.
func PairsBetween(rows [][]float32, qSizes []int32, library [][]float32, lSizes []int32, threshold float32, exclude []int64) (rowPtr []int64, col []int32, val []float32, err error) {
	raw, e := Ctx()
	if e != nil {
		return nil, nil, nil, e
	}
	nq, n, d := len(rows), len(library), 0
	if nq > 0 {
		d = len(rows[0])
	}
	if (qSizes != nil && len(qSizes) != nq) || (lSizes != nil && len(lSizes) != n) || (exclude != nil && len(exclude) != nq) {
		return nil, nil, nil, fmt.Errorf("sizes or exclude do not match %d rows and %d library rows", nq, n)
	}
	rowPtr = make([]int64, nq+1)
	if nq == 0 || n == 0 { // an empty side, no row length to pass: the empty list, as the Python mirror returns it
		return rowPtr, nil, nil, nil
	}
	flatQ, flatL := flatRows(rows, d), flatRows(library, d)
	i32 := func(s []int32) *C.int32_t {
		if len(s) == 0 {
			return nil
		}
		return (*C.int32_t)(unsafe.Pointer(&s[0]))
	}
	var ex *C.int64_t
	if len(exclude) > 0 {
		ex = (*C.int64_t)(unsafe.Pointer(&exclude[0]))
	}
	total := C.int64_t(-1)
	call := func(c *C.int32_t, v *C.float, cap int64) C.int {
		return C.icl_pairs_between((*C.icl_ctx)(raw), (*C.float)(unsafe.Pointer(&flatQ[0])), i32(qSizes), C.int64_t(nq),
			(*C.float)(unsafe.Pointer(&flatL[0])), i32(lSizes), C.int64_t(n), C.int32_t(d), C.float(threshold), ex,
			(*C.int64_t)(unsafe.Pointer(&rowPtr[0])), c, v, C.int64_t(cap), &total)
	}
	if rc := call(nil, nil, 0); rc != C.ICL_OK {
		return nil, nil, nil, fmt.Errorf("%s", C.GoString(C.icl_last_error((*C.icl_ctx)(raw))))
	}
	t := int64(total)
	col, val = make([]int32, t+1), make([]float32, t+1)
	if t > 0 {
		if rc := call((*C.int32_t)(unsafe.Pointer(&col[0])), (*C.float)(unsafe.Pointer(&val[0])), t); rc != C.ICL_OK {
			return nil, nil, nil, fmt.Errorf("%s", C.GoString(C.icl_last_error((*C.icl_ctx)(raw))))
		}
	}
	return rowPtr, col[:t], val[:t], nil
}

// PairGroups is icl_pair_groups (host only): the connected components of the pair graph of a CSR list: group[i] is the smallest index
// of i's component, nGroups the number of components with at least two members.
func PairGroups(rowPtr []int64, col []int32) (group []int32, nGroups int, err error) {
	if len(rowPtr) == 0 {
		return nil, 0, fmt.Errorf("rowPtr needs n + 1 entries")
	}
	n := len(rowPtr) - 1
	group = make([]int32, n+1)
	var c *C.int32_t
	if len(col) > 0 {
		c = (*C.int32_t)(unsafe.Pointer(&col[0]))
	}
	var ng C.int64_t
	if rc := C.icl_pair_groups(C.int64_t(n), (*C.int64_t)(unsafe.Pointer(&rowPtr[0])), c, (*C.int32_t)(unsafe.Pointer(&group[0])), &ng); rc != C.ICL_OK {
		return nil, 0, fmt.Errorf("icl_pair_groups: malformed pair list")
	}
	return group[:n], int(ng), nil
}

// Where a qualifying PNG of the batched file calls is inflated and unfiltered: icl_set_png_options' modes.
const (
	PNGHost = int(C.ICL_PNG_HOST)
	PNGGPU  = int(C.ICL_PNG_GPU)
)

// SetPNGOptions chooses whether the batched file calls (ClusterRequests and the embedding calls behind it) decode qualifying PNGs on the
// GPU (same rows, status codes and messages in both modes).
func SetPNGOptions(pngMode int) error {
	raw, e := Ctx()
	if e != nil {
		return e
	}
	if rc := C.icl_set_png_options((*C.icl_ctx)(raw), C.int(pngMode)); rc != C.ICL_OK {
		return fmt.Errorf("%s", C.GoString(C.icl_last_error((*C.icl_ctx)(raw))))
	}
	return nil
}

// LastPNGStats reports what the last batched file call did with its PNGs: decoded on the GPU, decoded by the host because of the routing
// rule, rejected by the GPU check and redone by the host, zlib stream bytes uploaded.
func LastPNGStats() (gpuPNGs, hostPNGs, redoneOnHost, streamBytes int64, err error) {
	raw, e := Ctx()
	if e != nil {
		return 0, 0, 0, 0, e
	}
	var a, b, c, d C.int64_t
	if rc := C.icl_last_png_stats((*C.icl_ctx)(raw), &a, &b, &c, &d); rc != C.ICL_OK {
		return 0, 0, 0, 0, fmt.Errorf("%s", C.GoString(C.icl_last_error((*C.icl_ctx)(raw))))
	}
	return int64(a), int64(b), int64(c), int64(d), nil
}

// Request is one workflow.Run call's input as icl_cluster_requests takes it: the image files, each image's label columns within
// the request's label set (GenerateLabelVector's indices; -1 for a label the set does not hold) and the size constraints.
type Request struct {
	Paths   []string
	Labels  [][]int32 // per image
	NLabels int       // len(LabelSet)
	MinSize int
	MaxSize int
}

// RequestResult is one request's outcome: Status is ICL_OK, ICL_ERR_CONSTRAINT (the reference's (nil,false)) or the code of its
// lowest failed file; ClusterID / MemberRank are per image (-1 rows when the request failed).
type RequestResult struct {
	Status     int
	ClusterID  []int32
	MemberRank []int32
	NClusters  int
}

// ClusterRequests runs createEmbeddings + PerformClusteringWithConstraints (workflow.go:84-94) for every request in ONE engine
// call (icl_cluster_requests): the combined embeddings are assembled on the GPU and never cross PCIe.  head: ICL_HEAD_DENSE0 or
// ICL_HEAD_POOLED; prec: ICL_PREC_*; threads: host decode threads (0 = up to 16).  The returned error names the lowest failed
// request; the results of the others are valid beside it.
func ClusterRequests(reqs []Request, head, prec, threads int) ([]RequestResult, error) {
	raw, e := Ctx()
	if e != nil {
		return nil, e
	}
	if len(reqs) == 0 {
		return nil, nil
	}
	var paths []*C.char
	defer func() {
		for _, p := range paths {
			C.free(unsafe.Pointer(p))
		}
	}()
	n := make([]C.int32_t, len(reqs))
	nl := make([]C.int32_t, len(reqs))
	mn := make([]C.int32_t, len(reqs))
	mx := make([]C.int32_t, len(reqs))
	off := []C.int64_t{0}
	idx := []C.int32_t{}
	for r, q := range reqs {
		if len(q.Labels) != len(q.Paths) {
			return nil, fmt.Errorf("request %d: %d paths, %d label lists", r, len(q.Paths), len(q.Labels))
		}
		n[r], nl[r], mn[r], mx[r] = C.int32_t(len(q.Paths)), C.int32_t(q.NLabels), C.int32_t(q.MinSize), C.int32_t(q.MaxSize)
		for i, p := range q.Paths {
			paths = append(paths, C.CString(p))
			for _, j := range q.Labels[i] {
				idx = append(idx, C.int32_t(j))
			}
			off = append(off, C.int64_t(len(idx)))
		}
	}
	rows := len(paths)
	cid := make([]C.int32_t, rows+1)
	rank := make([]C.int32_t, rows+1)
	nc := make([]C.int32_t, len(reqs))
	nm := make([]C.int32_t, len(reqs))
	st := make([]C.int32_t, len(reqs))
	for r := range st {
		st[r] = -1 // stays -1 when the call fails before the requests run
	}
	paths = append(paths, nil) // (never read: keeps &paths[0] valid for a call without images)
	idx = append(idx, 0)
	rc := C.icl_cluster_requests((*C.icl_ctx)(raw), C.int32_t(len(reqs)), (**C.char)(unsafe.Pointer(&paths[0])), &n[0], &nl[0], &off[0], &idx[0],
		&mn[0], &mx[0], C.int(head), C.int(prec), C.int32_t(threads), &cid[0], &rank[0], &nc[0], &nm[0], nil, &st[0], nil, nil)
	paths = paths[:rows]
	var callErr error
	if rc != C.ICL_OK {
		callErr = fmt.Errorf("%s", C.GoString(C.icl_last_error((*C.icl_ctx)(raw))))
		if st[0] < 0 { // still the -1 put there: an argument or device error, status untouched (imageclust.h), no per-request results
			return nil, callErr
		}
	}
	out := make([]RequestResult, len(reqs))
	at := 0
	for r, q := range reqs {
		k := len(q.Paths)
		out[r] = RequestResult{Status: int(st[r]), NClusters: int(nc[r]), ClusterID: make([]int32, k), MemberRank: make([]int32, k)}
		for i := 0; i < k; i++ {
			out[r].ClusterID[i], out[r].MemberRank[i] = int32(cid[at+i]), int32(rank[at+i])
		}
		at += k
	}
	return out, callErr
}

// RequestBytes is Request for a caller that holds the encoded images (models.UploadedImage.Data, workflow.go:66) instead of files.
type RequestBytes struct {
	Images  [][]byte  // each the bytes of a JPEG / PNG / PPM file; an empty one fails that image, not the call
	Labels  [][]int32 // per image
	NLabels int
	MinSize int
	MaxSize int
}

// ClusterRequestsBytes is ClusterRequests over images held in memory (icl_cluster_requests_mem): nothing is written to disk for the
// engine's sake.  The slices are handed to C in place: they are pinned for the duration of the call and must not be changed until
// it returns.  The pointer and length arrays live in C memory (a Go slice of Go pointers must not cross cgo).  Results, statuses and
// the returned error are ClusterRequests' on the same bytes; a message names an image as "image <i> (in memory, <n> bytes)".
func ClusterRequestsBytes(reqs []RequestBytes, head, prec, threads int) ([]RequestResult, error) {
	raw, e := Ctx()
	if e != nil {
		return nil, e
	}
	if len(reqs) == 0 {
		return nil, nil
	}
	rows := 0
	for r, q := range reqs {
		if len(q.Labels) != len(q.Images) {
			return nil, fmt.Errorf("request %d: %d images, %d label lists", r, len(q.Images), len(q.Labels))
		}
		rows += len(q.Images)
	}
	ptrSize := C.size_t(unsafe.Sizeof(uintptr(0)))
	datav := (**C.uint8_t)(C.calloc(C.size_t(rows+1), ptrSize))
	defer C.free(unsafe.Pointer(datav))
	bytesv := (*C.int64_t)(C.calloc(C.size_t(rows+1), 8))
	defer C.free(unsafe.Pointer(bytesv))
	data, size := unsafe.Slice(datav, rows+1), unsafe.Slice(bytesv, rows+1)
	var pin runtime.Pinner
	defer pin.Unpin()
	n := make([]C.int32_t, len(reqs))
	nl := make([]C.int32_t, len(reqs))
	mn := make([]C.int32_t, len(reqs))
	mx := make([]C.int32_t, len(reqs))
	off := []C.int64_t{0}
	idx := []C.int32_t{}
	at := 0
	for r, q := range reqs {
		n[r], nl[r], mn[r], mx[r] = C.int32_t(len(q.Images)), C.int32_t(q.NLabels), C.int32_t(q.MinSize), C.int32_t(q.MaxSize)
		for i, img := range q.Images {
			if len(img) > 0 { // (an empty image stays NULL / 0: the engine reports it as that image's failure)
				pin.Pin(&img[0])
				data[at], size[at] = (*C.uint8_t)(unsafe.Pointer(&img[0])), C.int64_t(len(img))
			}
			at++
			for _, j := range q.Labels[i] {
				idx = append(idx, C.int32_t(j))
			}
			off = append(off, C.int64_t(len(idx)))
		}
	}
	cid := make([]C.int32_t, rows+1)
	rank := make([]C.int32_t, rows+1)
	nc := make([]C.int32_t, len(reqs))
	nm := make([]C.int32_t, len(reqs))
	st := make([]C.int32_t, len(reqs))
	for r := range st {
		st[r] = -1 // stays -1 when the call fails before the requests run
	}
	idx = append(idx, 0)
	rc := C.icl_cluster_requests_mem((*C.icl_ctx)(raw), C.int32_t(len(reqs)), datav, bytesv, &n[0], &nl[0], &off[0], &idx[0],
		&mn[0], &mx[0], C.int(head), C.int(prec), C.int32_t(threads), &cid[0], &rank[0], &nc[0], &nm[0], nil, &st[0], nil, nil)
	var callErr error
	if rc != C.ICL_OK {
		callErr = fmt.Errorf("%s", C.GoString(C.icl_last_error((*C.icl_ctx)(raw))))
		if st[0] < 0 { // an argument or device error: status untouched (imageclust.h), no per-request results
			return nil, callErr
		}
	}
	out := make([]RequestResult, len(reqs))
	at = 0
	for r, q := range reqs {
		k := len(q.Images)
		out[r] = RequestResult{Status: int(st[r]), NClusters: int(nc[r]), ClusterID: make([]int32, k), MemberRank: make([]int32, k)}
		for i := 0; i < k; i++ {
			out[r].ClusterID[i], out[r].MemberRank[i] = int32(cid[at+i]), int32(rank[at+i])
		}
		at += k
	}
	return out, callErr
}

// LastRequestsMs reports the stage wall times of the last ClusterRequests: files -> embedding rows, assembly, clustering.
func LastRequestsMs() (embedMs, assembleMs, clusterMs float64, err error) {
	raw, e := Ctx()
	if e != nil {
		return 0, 0, 0, e
	}
	var a, b, c C.double
	if rc := C.icl_last_requests_ms((*C.icl_ctx)(raw), &a, &b, &c); rc != C.ICL_OK {
		return 0, 0, 0, fmt.Errorf("%s", C.GoString(C.icl_last_error((*C.icl_ctx)(raw))))
	}
	return float64(a), float64(b), float64(c), nil
}

// The limits of resizeImageIfNeeded (internal/rekognition/rekognition.go: MaxImageSize, and the box it resizes into).
const (
	MaxImageSize = 5 * 1024 * 1024
	MaxImageDim  = 2048
)

// DownsizeImage is resizeImageIfNeeded (rekognition.go:173-259) on the host (icl_downsize_image_mem): an image of at most MaxImageSize
// bytes comes back as it is, a larger one decoded, resized into the 2048 box -- with the reference's rows / columns swap: a 4000x3000
// landscape photo becomes 1536 wide x 2048 high -- and written as a JPEG at quality 95, once more at half the size if it is still too
// large.  No GPU is touched.
func DownsizeImage(data []byte) ([]byte, error) {
	if len(data) == 0 {
		return nil, fmt.Errorf("empty image buffer")
	}
	var need C.int64_t
	p := (*C.uint8_t)(unsafe.Pointer(&data[0]))
	out := make([]byte, len(data)) // (a downsized image is rarely larger than its source; a second call only if it is)
	for try := 0; try < 2; try++ {
		rc := C.icl_downsize_image_mem(p, C.int64_t(len(data)), MaxImageSize, MaxImageDim, (*C.uint8_t)(unsafe.Pointer(&out[0])), C.int64_t(len(out)), &need, nil)
		if rc == C.ICL_OK {
			return out[:need], nil
		}
		if rc != C.ICL_ERR_ARG || int(need) <= len(out) {
			break
		}
		out = make([]byte, int(need))
	}
	return nil, fmt.Errorf("%s", C.GoString(C.icl_last_error(nil)))
}

// DownsizeImages is DownsizeImage over a list in one call (icl_downsize_images_mem): JPEGs above the limit are rebuilt, resized and
// encoded on the GPU.  Result i is image i's, byte-equal to DownsizeImage's; status[i] != 0 marks an image that failed alone (its
// result is empty), and the returned error then names the lowest failed index.  The slices are handed to C in place.
func DownsizeImages(images [][]byte, threads int) (out [][]byte, status []int32, err error) {
	raw, e := Ctx()
	if e != nil {
		return nil, nil, e
	}
	n := len(images)
	if n == 0 {
		return nil, nil, nil
	}
	ptrSize := C.size_t(unsafe.Sizeof(uintptr(0)))
	datav := (**C.uint8_t)(C.calloc(C.size_t(n+1), ptrSize))
	defer C.free(unsafe.Pointer(datav))
	bytesv := (*C.int64_t)(C.calloc(C.size_t(n+1), 8))
	defer C.free(unsafe.Pointer(bytesv))
	data, size := unsafe.Slice(datav, n+1), unsafe.Slice(bytesv, n+1)
	var pin runtime.Pinner
	defer pin.Unpin()
	capBytes := int64(1)
	for i, img := range images {
		if len(img) > 0 {
			pin.Pin(&img[0])
			data[i], size[i] = (*C.uint8_t)(unsafe.Pointer(&img[0])), C.int64_t(len(img))
			capBytes += int64(len(img))
		}
	}
	st := make([]C.int32_t, n)
	off := make([]C.int64_t, n+1)
	var buf []byte
	var rc C.int
	for try := 0; try < 2; try++ { // (an output is rarely larger than its input; the call says what it needs when one is)
		buf = make([]byte, capBytes)
		rc = C.icl_downsize_images_mem((*C.icl_ctx)(raw), datav, bytesv, C.int64_t(n), MaxImageSize, MaxImageDim, C.int32_t(threads),
			(*C.uint8_t)(unsafe.Pointer(&buf[0])), C.int64_t(capBytes), &off[0], &st[0])
		if rc == C.ICL_ERR_ARG && int64(off[n]) > capBytes {
			capBytes = int64(off[n])
			continue
		}
		break
	}
	if rc != C.ICL_OK {
		err = fmt.Errorf("%s", C.GoString(C.icl_last_error((*C.icl_ctx)(raw))))
		failed := false
		for _, s := range st {
			failed = failed || s != 0
		}
		if !failed { // an argument or device error: no per-image results
			return nil, nil, err
		}
	}
	out, status = make([][]byte, n), make([]int32, n)
	for i := range images {
		out[i], status[i] = buf[off[i]:off[i+1]], int32(st[i])
	}
	return out, status, err
}
