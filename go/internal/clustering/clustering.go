// Package clustering: drop-in replacement of imageclust/internal/clustering backed by libimageclust_hip.so.
// Same exported names and signatures as the reference's clustering.go; the arithmetic runs on the GPU through
// the C-ABI of include/imageclust.h.  NOT COMPILED in the authoring container (no Go toolchain): logic-free glue.
package clustering

/*
#cgo CFLAGS: -I${SRCDIR}/../../../include
#cgo LDFLAGS: -L${SRCDIR}/../../../imageclust_amd -limageclust_hip
#include <stdlib.h>
#include "imageclust.h"
*/
import "C"

import (
	"fmt"
	"log"
	"sort"
	"unsafe"

	"imageclust/internal/iclengine"
)

// Cluster mirrors clustering.go:11-15.
type Cluster struct {
	Indices  []int
	Size     int
	Centroid []float32
}

// engine: the context shared with internal/embeddings (one GPU context and workspace per process).
func engine() (*C.icl_ctx, error) {
	p, err := iclengine.Ctx()
	return (*C.icl_ctx)(p), err
}

// NewCluster: clustering.go:18-26 (plain Go, unchanged).
func NewCluster(index int, embedding []float32) Cluster {
	c := make([]float32, len(embedding))
	copy(c, embedding)
	return Cluster{Indices: []int{index}, Size: 1, Centroid: c}
}

// RemoveClusters: clustering.go:51-58 (plain Go, unchanged).
func RemoveClusters(clusters []Cluster, i, j int) []Cluster {
	if i > j {
		i, j = j, i
	}
	clusters = append(clusters[:j], clusters[j+1:]...)
	clusters = append(clusters[:i], clusters[i+1:]...)
	return clusters
}

// MergeClusters: clustering.go:29-47; the centroid comes from icl_merge_centroid.
func MergeClusters(a, b Cluster) Cluster {
	e, err := engine()
	if err != nil {
		log.Panic(err)
	}
	out := make([]float32, len(a.Centroid))
	if len(out) > 0 {
		if rc := C.icl_merge_centroid(e, (*C.float)(unsafe.Pointer(&a.Centroid[0])), C.int64_t(a.Size),
			(*C.float)(unsafe.Pointer(&b.Centroid[0])), C.int64_t(b.Size), C.int32_t(len(out)), (*C.float)(unsafe.Pointer(&out[0]))); rc != C.ICL_OK {
			log.Panicf("icl_merge_centroid: %s", C.GoString(C.icl_last_error(e))) // never a silent zero centroid
		}
	}
	return Cluster{Indices: append(append([]int{}, a.Indices...), b.Indices...), Size: a.Size + b.Size, Centroid: out}
}

func flatten(clusters []Cluster) (flat []float32, sizes []int32, d int) {
	if len(clusters) == 0 {
		return nil, nil, 0
	}
	d = len(clusters[0].Centroid)
	flat = make([]float32, len(clusters)*d) // [][]float32 cannot cross cgo: one contiguous buffer
	sizes = make([]int32, len(clusters))
	for i, c := range clusters {
		copy(flat[i*d:(i+1)*d], c.Centroid)
		sizes[i] = int32(c.Size)
	}
	return
}

// ComputeInitialDistanceMatrix: clustering.go:61-73 -> icl_ward_distance_matrix.
func ComputeInitialDistanceMatrix(clusters []Cluster) [][]float32 {
	n := len(clusters)
	out := make([][]float32, n)
	if n == 0 {
		return out
	}
	e, err := engine()
	if err != nil {
		log.Panic(err)
	}
	flat, sizes, d := flatten(clusters)
	D := make([]float32, n*n)
	var cptr *C.float
	if d > 0 {
		cptr = (*C.float)(unsafe.Pointer(&flat[0]))
	}
	if rc := C.icl_ward_distance_matrix(e, cptr, (*C.int32_t)(unsafe.Pointer(&sizes[0])), C.int64_t(n), C.int32_t(d),
		(*C.float)(unsafe.Pointer(&D[0])), C.int64_t(n)); rc != C.ICL_OK {
		log.Panicf("icl_ward_distance_matrix: %s", C.GoString(C.icl_last_error(e)))
	}
	for i := range out {
		out[i] = D[i*n : (i+1)*n : (i+1)*n]
	}
	return out
}

// FindClosestClusters: clustering.go:119-133 -> icl_find_closest.
func FindClosestClusters(distanceMatrix [][]float32) (int, int) {
	n := len(distanceMatrix)
	if n < 2 {
		return -1, -1
	}
	e, err := engine()
	if err != nil {
		log.Panic(err)
	}
	flat := make([]float32, n*n)
	for i, row := range distanceMatrix {
		copy(flat[i*n:(i+1)*n], row)
	}
	var i, j C.int64_t
	if rc := C.icl_find_closest(e, (*C.float)(unsafe.Pointer(&flat[0])), C.int64_t(n), C.int64_t(n), &i, &j); rc != C.ICL_OK {
		log.Panicf("icl_find_closest: %s", C.GoString(C.icl_last_error(e)))
	}
	return int(i), int(j)
}

// UpdateDistanceMatrix: clustering.go:76-96 -> icl_update_distance_matrix (rows/columns removedIdx1, removedIdx2 dropped
// order-preserving, new last row/column from the centroids).  clusters is the list AFTER RemoveClusters + append (:240-241).
func UpdateDistanceMatrix(distanceMatrix [][]float32, clusters []Cluster, newCluster Cluster, removedIdx1, removedIdx2 int) [][]float32 {
	n := len(distanceMatrix)
	e, err := engine()
	if err != nil {
		log.Panic(err)
	}
	flatD := make([]float32, n*n)
	for i, row := range distanceMatrix {
		copy(flatD[i*n:(i+1)*n], row)
	}
	flatC, sizes, d := flatten(clusters)
	m := n - 1
	out := make([]float32, m*m)
	var cptr *C.float
	if d > 0 {
		cptr = (*C.float)(unsafe.Pointer(&flatC[0]))
	}
	if rc := C.icl_update_distance_matrix(e, (*C.float)(unsafe.Pointer(&flatD[0])), C.int64_t(n), C.int64_t(n), cptr,
		(*C.int32_t)(unsafe.Pointer(&sizes[0])), C.int32_t(d), C.int64_t(removedIdx1), C.int64_t(removedIdx2),
		(*C.float)(unsafe.Pointer(&out[0])), C.int64_t(m)); rc != C.ICL_OK {
		log.Panicf("icl_update_distance_matrix: %s", C.GoString(C.icl_last_error(e)))
	}
	res := make([][]float32, m)
	for i := range res {
		res[i] = out[i*m : (i+1)*m : (i+1)*m]
	}
	return res
}

// RemoveRowsAndColumns: clustering.go:100-116 (plain Go, unchanged).
func RemoveRowsAndColumns(matrix [][]float32, i, j int) [][]float32 {
	if i > j {
		i, j = j, i
	}
	for idx := range matrix {
		matrix[idx] = append(matrix[idx][:j], matrix[idx][j+1:]...)
		matrix[idx] = append(matrix[idx][:i], matrix[idx][i+1:]...)
	}
	matrix = append(matrix[:j], matrix[j+1:]...)
	matrix = append(matrix[:i], matrix[i+1:]...)
	return matrix
}

// DotFloat32: clustering.go:148-157 (plain Go, unchanged: in-order fp32 sum, panics on length mismatch).
func DotFloat32(a, b []float32) float32 {
	if len(a) != len(b) {
		panic("Vectors must be the same length")
	}
	var sum float32
	for i := range a {
		sum += a[i] * b[i]
	}
	return sum
}

// WardDistance: clustering.go:136-145 (a 2x2 call of the exact distance tile).
func WardDistance(a, b Cluster) float32 {
	return ComputeInitialDistanceMatrix([]Cluster{a, b})[1][0]
}

// CalculateOptimalClusters: clustering.go:168-186.
func CalculateOptimalClusters(totalItems, minSize, maxSize int) (int, error) {
	var k C.int64_t
	if rc := C.icl_calc_optimal_clusters(C.int64_t(totalItems), C.int64_t(minSize), C.int64_t(maxSize), &k); rc != C.ICL_OK {
		if totalItems < minSize {
			return 0, fmt.Errorf("total items (%d) less than minimum cluster size (%d)", totalItems, minSize)
		}
		return 0, fmt.Errorf("cannot satisfy cluster size constraints with total items (%d), minSize (%d), and maxSize (%d)", totalItems, minSize, maxSize)
	}
	return int(k), nil
}

// PerformClusteringWithConstraints: clustering.go:198-284 -> icl_cluster (exact update: bit-identical ids).
func PerformClusteringWithConstraints(embeddings [][]float32, productReferenceIDs []string, minSize, maxSize int) (map[int][]string, bool) {
	n := len(embeddings)
	log.Printf("Total items for clustering: %d", n)
	e, err := engine()
	if err != nil {
		log.Printf("Clustering engine error: %v", err)
		return nil, false
	}
	d := 0
	if n > 0 {
		d = len(embeddings[0])
	}
	flat := make([]float32, n*d)
	for i, row := range embeddings {
		copy(flat[i*d:(i+1)*d], row)
	}
	cid := make([]int32, n+1)
	rank := make([]int32, n+1)
	var nc C.int32_t
	var eptr *C.float
	if len(flat) > 0 {
		eptr = (*C.float)(unsafe.Pointer(&flat[0]))
	}
	rc := C.icl_cluster(e, eptr, C.int64_t(n), C.int32_t(d), C.int32_t(minSize), C.int32_t(maxSize), C.ICL_UPDATE_EXACT,
		(*C.int32_t)(unsafe.Pointer(&cid[0])), (*C.int32_t)(unsafe.Pointer(&rank[0])), &nc)
	if rc != C.ICL_OK {
		log.Printf("Clustering constraint error: %s", C.GoString(C.icl_last_error(e)))
		return nil, false
	}
	clusterMap := make(map[int][]string, int(nc))
	sizes := make([]int, int(nc))
	for i := 0; i < n; i++ {
		if cid[i] >= 0 {
			sizes[cid[i]]++
		}
	}
	for c, s := range sizes {
		clusterMap[c] = make([]string, s)
	}
	for i := 0; i < n; i++ {
		if cid[i] >= 0 {
			clusterMap[int(cid[i])][rank[i]] = productReferenceIDs[i]
		}
	}
	log.Printf("Clustering successful. Formed %d valid clusters.", len(clusterMap))
	return clusterMap, true
}

// ClusteringJob is one PerformClusteringWithConstraints call of a batch.
type ClusteringJob struct {
	Embeddings          [][]float32
	ProductReferenceIDs []string
	MinSize, MaxSize    int
}

// ClusteringResult is what PerformClusteringWithConstraints returns for one job.
type ClusteringResult struct {
	Clusters map[int][]string
	OK       bool
}

// PerformClusteringWithConstraintsBatch runs many independent PerformClusteringWithConstraints calls (exact mode) in one
// icl_cluster_many call; result j equals PerformClusteringWithConstraints(jobs[j]...).
func PerformClusteringWithConstraintsBatch(jobs []ClusteringJob) []ClusteringResult {
	out := make([]ClusteringResult, len(jobs))
	if len(jobs) == 0 {
		return out
	}
	e, err := engine()
	if err != nil {
		log.Printf("Clustering engine error: %v", err)
		return out
	}
	np := len(jobs)
	eoff := make([]int64, np)
	n := make([]int32, np)
	d := make([]int32, np)
	mn := make([]int32, np)
	mx := make([]int32, np)
	total, rows := 0, 0
	for j, job := range jobs {
		n[j] = int32(len(job.Embeddings))
		if n[j] > 0 {
			d[j] = int32(len(job.Embeddings[0]))
		}
		mn[j], mx[j] = int32(job.MinSize), int32(job.MaxSize)
		eoff[j] = int64(total)
		total += (int(n[j])*int(d[j]) + 3) / 4 * 4 // each problem on a 16-byte boundary
		rows += int(n[j])
	}
	flat := make([]float32, total+1) // [][]float32 cannot cross cgo: one contiguous buffer
	for j, job := range jobs {
		for i, row := range job.Embeddings {
			copy(flat[int(eoff[j])+i*int(d[j]):], row)
		}
	}
	cid := make([]int32, rows+1)
	rank := make([]int32, rows+1)
	nc := make([]int32, np)
	nm := make([]int32, np)
	st := make([]int32, np)
	for j := range st {
		st[j] = -1 // stays -1 when the call fails before the problems run (a bad argument, no device memory)
	}
	rc := C.icl_cluster_many(e, C.int32_t(np), (*C.float)(unsafe.Pointer(&flat[0])), C.int64_t(len(flat)),
		(*C.int64_t)(unsafe.Pointer(&eoff[0])), (*C.int32_t)(unsafe.Pointer(&n[0])), (*C.int32_t)(unsafe.Pointer(&d[0])),
		(*C.int32_t)(unsafe.Pointer(&mn[0])), (*C.int32_t)(unsafe.Pointer(&mx[0])), (*C.int32_t)(unsafe.Pointer(&cid[0])),
		(*C.int32_t)(unsafe.Pointer(&rank[0])), (*C.int32_t)(unsafe.Pointer(&nc[0])), (*C.int32_t)(unsafe.Pointer(&nm[0])), nil,
		(*C.int32_t)(unsafe.Pointer(&st[0])))
	if rc != C.ICL_OK {
		log.Printf("Clustering batch: %s", C.GoString(C.icl_last_error(e)))
	}
	off := 0
	for j, job := range jobs {
		if st[j] == C.ICL_OK {
			clusterMap := make(map[int][]string, int(nc[j]))
			sizes := make([]int, int(nc[j]))
			for i := 0; i < int(n[j]); i++ {
				if c := cid[off+i]; c >= 0 {
					sizes[c]++
				}
			}
			for c, s := range sizes {
				clusterMap[c] = make([]string, s)
			}
			for i := 0; i < int(n[j]); i++ {
				if c := cid[off+i]; c >= 0 {
					clusterMap[int(c)][rank[off+i]] = job.ProductReferenceIDs[i]
				}
			}
			out[j] = ClusteringResult{Clusters: clusterMap, OK: true}
		}
		off += int(n[j])
	}
	return out
}

// ResumeClustering goes on from clusters that exist (the loop of PerformClusteringWithConstraints, :216-246, started from them instead
// of from singletons): centroids[i] and sizes[i] describe cluster i -- a new image is a cluster of size 1 with its embedding, a negative
// size freezes the cluster -- and kTarget > 0 replaces CalculateOptimalClusters.  The result is at seed granularity
// (iclengine.SeededResult); false on impossible constraints, as the reference's (nil, false).
func ResumeClustering(centroids [][]float32, sizes []int32, minSize, maxSize, kTarget int) (iclengine.SeededResult, bool) {
	return ResumeClusteringApart(centroids, sizes, minSize, maxSize, kTarget, nil, nil)
}

// The update choice of ResumeClusteringUpdate: the exact pipeline (ResumeClustering), or FAST mode (ICL_UPDATE_LW).
const (
	UpdateExact = 0
	UpdateLW    = 1
)

// ResumeClusteringUpdate is ResumeClustering with the update mode chosen: UpdateExact is ResumeClustering; UpdateLW resumes in FAST mode
// (iclengine.ClusterSeededFast, icl_cluster_seeded_fast on the large-N engine whatever the number of clusters: the one-workgroup routes
// have no FAST form).  A FAST run resumed from its clusters is not the uncut FAST run, and FAST mode takes no keep-apart constraints.
func ResumeClusteringUpdate(centroids [][]float32, sizes []int32, minSize, maxSize, kTarget, update int) (iclengine.SeededResult, bool) {
	if update != UpdateLW {
		return ResumeClustering(centroids, sizes, minSize, maxSize, kTarget)
	}
	res, err := iclengine.ClusterSeededFast(iclengine.SeededProblem{Centroids: centroids, Sizes: sizes, MinSize: minSize, MaxSize: maxSize, KTarget: kTarget})
	if err != nil {
		log.Printf("Clustering engine error: %v", err)
		return iclengine.SeededResult{}, false
	}
	if res.Status != 0 {
		log.Printf("Seeded clustering failed with status %d: %s", res.Status, iclengine.LastError())
		return res, false
	}
	return res, true
}

// ResumeClusteringApart is ResumeClustering with keep-apart constraints (iclengine.ClusterManyApart, icl_cluster_many_apart; above
// iclengine.ManySeededMax clusters iclengine.ClusterApart, icl_cluster_apart on the large-N engine): apartPairs
// lists cluster indices that must never share a cluster, apartClass (one int per cluster, 0: none) classes whose members must not --
// class 1 on every kept cluster, with kTarget their number, lets the kept clusters take the leftovers but not each other.  A merged
// cluster inherits the bans of both parents, so the loop may end before kTarget clusters are reached.  With both lists empty it is
// ResumeClustering, whatever the number of clusters.
func ResumeClusteringApart(centroids [][]float32, sizes []int32, minSize, maxSize, kTarget int, apartPairs [][2]int32,
	apartClass []int32) (iclengine.SeededResult, bool) {
	pr := iclengine.SeededProblem{Centroids: centroids, Sizes: sizes, MinSize: minSize, MaxSize: maxSize, KTarget: kTarget}
	var res []iclengine.SeededResult
	var err error
	constrained := len(apartPairs) > 0
	for _, c := range apartClass {
		constrained = constrained || c != 0
	}
	if constrained && len(sizes) > iclengine.ManySeededMax { // above the one-workgroup routes' cap: the large-N engine's constrained call
		var one iclengine.SeededResult
		one, err = iclengine.ClusterApart(iclengine.ApartProblem{SeededProblem: pr, ApartClass: apartClass, ApartPairs: apartPairs})
		res = []iclengine.SeededResult{one}
	} else if constrained {
		res, err = iclengine.ClusterManyApart([]iclengine.ApartProblem{{SeededProblem: pr, ApartClass: apartClass, ApartPairs: apartPairs}})
	} else if len(sizes) > iclengine.ManySeededMax { // above the one-workgroup routes' cap: the large-N engine's seeded call
		var one iclengine.SeededResult
		one, err = iclengine.ClusterSeeded(pr)
		res = []iclengine.SeededResult{one}
	} else {
		res, err = iclengine.ClusterManySeeded([]iclengine.SeededProblem{pr})
	}
	if err != nil {
		log.Printf("Clustering engine error: %v", err)
		return iclengine.SeededResult{}, false
	}
	if res[0].Status != 0 {
		log.Printf("Seeded clustering failed with status %d: %s", res[0].Status, iclengine.LastError())
		return res[0], false
	}
	return res[0], true
}

// NearestClusters answers, before ResumeClustering is asked to recluster: for each query cluster (a new image is a cluster of size 1
// with its embedding; nil qSizes: all singletons) which of the existing clusters are closest in the loop's own cost, and by how much
// (iclengine.Nearest -> icl_nearest: WardDistance of :136-157 bit for bit, no distance matrix).  maxSize > 0 leaves out the clusters
// the loop would refuse to merge the query with (:228).  idx[i] lists up to k positions in `clusters`, nearest first, ties by
// position; a row with fewer than k candidates ends in -1 (val MaxFloat32).
func NearestClusters(queries [][]float32, qSizes []int32, clusters []Cluster, k, maxSize int) (idx [][]int32, val [][]float32, err error) {
	centroids := make([][]float32, len(clusters))
	sizes := make([]int32, len(clusters))
	for i, c := range clusters {
		centroids[i] = c.Centroid
		sizes[i] = int32(c.Size)
	}
	return iclengine.Nearest(queries, qSizes, centroids, sizes, k, maxSize, nil)
}

// ClusterFit answers, for images that are clustered already: how well does each sit in the cluster it is in, and which other clusters
// would take it at what price (iclengine.ClusterFit -> icl_cluster_fit: WardDistance of :136-157 bit for bit on both sides, so "closer
// to another cluster than to its own" is an exact statement).  rows[i] is a cluster of qSizes[i] items (nil: singletons) that belongs
// to clusters[clusterOf[i]] (-1: to none); frozen[j] marks a cluster that is measured as an own cluster and never offered as an
// alternative (nil: none frozen); maxSize > 0 leaves out the clusters the loop would refuse to merge the row with (:228).  The result
// also names each cluster's representative row (smallest own cost) and worst row.
func ClusterFit(rows [][]float32, qSizes []int32, clusterOf []int32, clusters []Cluster, frozen []bool, kAlt, maxSize int) (iclengine.FitResult, error) {
	centroids := make([][]float32, len(clusters))
	sizes := make([]int32, len(clusters))
	for i, c := range clusters {
		centroids[i] = c.Centroid
		sizes[i] = int32(c.Size)
		if frozen != nil && frozen[i] {
			sizes[i] = -sizes[i]
		}
	}
	return iclengine.ClusterFit(rows, qSizes, clusterOf, centroids, sizes, kAlt, maxSize)
}

// FoldCentroids builds clusters from member lists: groups[g] lists positions in embeddings, and cluster g gets those Indices, their
// count as Size and the Centroid MergeClusters (:29-47) leaves after merging the members one at a time in list order
// (iclengine.FoldCentroids -> icl_fold_centroids, bit for bit).  It is what editing a held clustering needs -- a cluster after an image
// was deleted or moved, a partition adopted from elsewhere (DESIGN.md "Editing a held clustering").
func FoldCentroids(embeddings [][]float32, groups [][]int) ([]Cluster, error) {
	lists := make([][]int32, len(groups))
	for g, list := range groups {
		lists[g] = make([]int32, len(list))
		for i, m := range list {
			lists[g][i] = int32(m)
		}
	}
	cen, total, err := iclengine.FoldCentroids(embeddings, nil, lists)
	if err != nil {
		return nil, err
	}
	out := make([]Cluster, len(groups))
	for g := range groups {
		out[g] = Cluster{Indices: append([]int(nil), groups[g]...), Size: int(total[g]), Centroid: cen[g]}
	}
	return out, nil
}

// DuplicatePair is one pair of images whose WardDistance as singletons is at most the threshold: A comes before B in the caller's list.
type DuplicatePair struct {
	A, B  string
	Value float32
}

// DuplicatePairs lists EVERY pair of images whose WardDistance as singletons is at most threshold (iclengine.PairsWithin ->
// icl_pairs_within: exact values, no cap on an image's partners, no distance matrix), each pair once, ordered by position.
func DuplicatePairs(embeddings [][]float32, ids []string, threshold float32) ([]DuplicatePair, error) {
	if len(embeddings) != len(ids) {
		return nil, fmt.Errorf("%d embeddings for %d ids", len(embeddings), len(ids))
	}
	rowPtr, col, val, err := iclengine.PairsWithin(embeddings, nil, threshold)
	if err != nil {
		return nil, err
	}
	type at struct {
		a, b int
		v    float32
	}
	found := make([]at, 0, len(col))
	for i := range ids {
		for p := rowPtr[i]; p < rowPtr[i+1]; p++ {
			found = append(found, at{int(col[p]), i, val[p]})
		}
	}
	sort.Slice(found, func(x, y int) bool { return found[x].a < found[y].a || (found[x].a == found[y].a && found[x].b < found[y].b) })
	out := make([]DuplicatePair, len(found))
	for q, f := range found {
		out[q] = DuplicatePair{A: ids[f.a], B: ids[f.b], Value: f.v}
	}
	return out, nil
}

// LibraryDuplicate is one pair (new image, held image) whose WardDistance as singletons is at most the threshold.
type LibraryDuplicate struct {
	New, Held string
	Value     float32
}

// DuplicatesOf lists EVERY pair (new image, held image) whose WardDistance as singletons is at most threshold (iclengine.PairsBetween ->
// icl_pairs_between: exact values, no cap on an image's partners, no distance matrix, the held images never compared with each other),
// ordered by the new image's position and then by the held image's.
func DuplicatesOf(newEmbeddings [][]float32, newIDs []string, embeddings [][]float32, ids []string, threshold float32) ([]LibraryDuplicate, error) {
	if len(newEmbeddings) != len(newIDs) || len(embeddings) != len(ids) {
		return nil, fmt.Errorf("%d embeddings for %d new ids, %d for %d held ids", len(newEmbeddings), len(newIDs), len(embeddings), len(ids))
	}
	rowPtr, col, val, err := iclengine.PairsBetween(newEmbeddings, nil, embeddings, nil, threshold, nil)
	if err != nil {
		return nil, err
	}
	out := make([]LibraryDuplicate, 0, len(col))
	for i := range newIDs {
		for p := rowPtr[i]; p < rowPtr[i+1]; p++ {
			out = append(out, LibraryDuplicate{New: newIDs[i], Held: ids[col[p]], Value: val[p]})
		}
	}
	return out, nil
}

// DuplicateGroups returns the connected components of DuplicatePairs' graph that have at least two members (iclengine.PairGroups ->
// icl_pair_groups): members in position order, groups ordered by their first member.
func DuplicateGroups(embeddings [][]float32, ids []string, threshold float32) ([][]string, error) {
	if len(embeddings) != len(ids) {
		return nil, fmt.Errorf("%d embeddings for %d ids", len(embeddings), len(ids))
	}
	rowPtr, col, _, err := iclengine.PairsWithin(embeddings, nil, threshold)
	if err != nil {
		return nil, err
	}
	group, _, err := iclengine.PairGroups(rowPtr, col)
	if err != nil {
		return nil, err
	}
	at := make(map[int32]int)
	var out [][]string
	for i, g := range group { // a group's first member is its smallest index: groups open in order of their first member
		if g == int32(i) {
			at[g] = len(out)
			out = append(out, nil)
		}
		out[at[g]] = append(out[at[g]], ids[i])
	}
	kept := out[:0]
	for _, m := range out {
		if len(m) >= 2 {
			kept = append(kept, m)
		}
	}
	return kept, nil
}
