"""Host-side mirror of the reference's internal/workflow/workflow.go over the HIP engine: workflow.Run (:84-94) for a queue of requests.

The reference serves one request at a time: createEmbeddings (:149-185) embeds every image and appends its one-hot label vector
(GenerateLabelVector + CombineEmbeddings), then PerformClusteringWithConstraints (:89) clusters the combined rows.  RunRequests does that
for many requests in ONE engine call (icl_cluster_requests): the files are decoded and embedded in slabs, the combined rows are assembled
on the GPU and clustered there, one workgroup per request; only cluster ids come back.  No CPU fallback.
"""
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .clustering import Clustering, clusters_as_map
from .embeddings import AppContext

Request = Tuple[Sequence[str], Sequence[str], Sequence[Sequence[str]], Dict[str, int], int, int]


def LabelIndices(labels: Sequence[str], labelSet: Dict[str, int]) -> List[int]:
    """The columns GenerateLabelVector (embeddings.go:166-174) sets for one image: labelSet[label], or -1 for a label the set does not
    hold (:169, ignored by the engine)."""
    return [int(labelSet.get(label, -1)) for label in labels]


def PackRequests(requests: Sequence[Request]):
    """requests -> what _lib.pack_requests takes: (paths, label indices per image, len(labelSet), minSize, maxSize) per request."""
    out = []
    for r, (paths, ids, labels_per_image, labelSet, minSize, maxSize) in enumerate(requests):
        if len(ids) != len(paths) or len(labels_per_image) != len(paths):
            raise ValueError("request %d: %d paths, %d ids, %d label lists" % (r, len(paths), len(ids), len(labels_per_image)))
        out.append((list(paths), [LabelIndices(labels, labelSet) for labels in labels_per_image], len(labelSet), minSize, maxSize))
    return out


def _results(requests_ids, res, statuses):
    out = []
    for ids, (cid, rank, _, st) in zip(requests_ids, res):
        if statuses is not None:
            statuses.append(int(st))
        out.append((clusters_as_map(cid, rank, list(ids)), True) if st == _lib.ICL_OK else (None, False))
    return out


def RunRequests(appCtx: AppContext, requests: Sequence[Request], prec: int = _lib.PREC_FP32, threads: int = 0,
                statuses: Optional[List[int]] = None) -> List[Tuple[Optional[Dict[int, List[str]]], bool]]:
    """workflow.go:84-94 for every request = (paths, ids, labels_per_image, labelSet, minSize, maxSize) -> [(map cluster id -> member ids,
    ok), ...], each entry what PerformClusteringWithConstraints returns for that request's combined embeddings: (None, False) when the
    constraints cannot be met -- and when one of the request's files cannot be read (workflow.go:162-181 fails the request; the others
    are unaffected).  `statuses`, when given, receives every request's ICL_* code."""
    if appCtx.Net is None or appCtx.Net.Empty():
        raise _lib.ICLError(_lib.ICL_ERR_NOMODEL, "RunRequests: no model loaded")
    res = appCtx.Net.ctx.cluster_requests(PackRequests(requests), appCtx.Head, prec, threads)
    return _results([r[1] for r in requests], res, statuses)


UploadedRequest = Tuple[Sequence[Tuple[str, bytes]], Sequence[Sequence[str]], Dict[str, int], int, int]


def RunUploaded(appCtx: AppContext, requests: Sequence[UploadedRequest], prec: int = _lib.PREC_FP32, threads: int = 0,
                statuses: Optional[List[int]] = None) -> List[Tuple[Optional[Dict[int, List[str]]], bool]]:
    """workflow.Run(uploadedImages) (workflow.go:66-94) for every request = (uploaded, labels_per_image, labelSet, minSize, maxSize),
    `uploaded` a list of (Filename, Data) pairs as models.UploadedImage holds them.  The bytes go to the engine as they are
    (icl_cluster_requests_mem): nothing is written to a temporary directory (workflow.go:120-127 does that for gocv.IMRead's sake).  Image
    i of a request gets the id "img_<i>" processImages assigns (workflow.go:140).  Returns what RunRequests returns."""
    if appCtx.Net is None or appCtx.Net.Empty():
        raise _lib.ICLError(_lib.ICL_ERR_NOMODEL, "RunUploaded: no model loaded")
    packed, ids = [], []
    for r, (uploaded, labels_per_image, labelSet, minSize, maxSize) in enumerate(requests):
        if len(labels_per_image) != len(uploaded):
            raise ValueError("request %d: %d images, %d label lists" % (r, len(uploaded), len(labels_per_image)))
        packed.append(([data for _, data in uploaded], [LabelIndices(labels, labelSet) for labels in labels_per_image], len(labelSet), minSize, maxSize))
        ids.append(["img_%d" % i for i in range(len(uploaded))])
    res = appCtx.Net.ctx.cluster_requests_mem(packed, appCtx.Head, prec, threads)
    return _results(ids, res, statuses)


def RunMore(appCtx: AppContext, state: Clustering, newRequestImages, prec: int = _lib.PREC_FP32,
            threads: int = 0, dedupe_threshold: Optional[float] = None, update: Optional[int] = None, remove_ids=None):
    """More images for a request that has been answered: newRequestImages = (paths, ids, labels_per_image, labelSet) with the
    labelSet of the request `state` came from (the combined rows must be as wide as the state's).  Only the new images are embedded
    and combined (createEmbeddings, workflow.go:149-185); they join the state as singletons and the loop goes on from the clusters
    held (Clustering.add, .recluster; a state with keep_apart constraints keeps them whatever its size: icl_cluster_many_apart up to
    2 048 held clusters, icl_cluster_apart above) -> (state.as_map(), True), or (None, False) when the constraints cannot be met or a file cannot
    be read (workflow.go:162-181 fails the request; the state is as it was then).  With dedupe_threshold, a new image that duplicates a
    held image or an earlier new image under that threshold does not join (Clustering.add(skip_duplicates=)), and the result has a
    third entry, the list [(skipped id, partner id, value), ...] (empty where the call fails before the images are compared).  update
    (UPDATE_EXACT / UPDATE_LW; None: as the state was made) sets the state's mode from this call on: UPDATE_LW resumes in FAST mode
    (icl_cluster_seeded_fast), where a state with keep_apart constraints raises ICLError(ICL_ERR_UNSUPPORTED).  remove_ids (None: nothing)
    names held images that leave the state (Clustering.remove) once the new files have been read and before the new images are added."""
    if appCtx.Net is None or appCtx.Net.Empty():
        raise _lib.ICLError(_lib.ICL_ERR_NOMODEL, "RunMore: no model loaded")
    paths, ids, labels_per_image, labelSet = newRequestImages
    if len(ids) != len(paths) or len(labels_per_image) != len(paths):
        raise ValueError("%d paths, %d ids, %d label lists" % (len(paths), len(ids), len(labels_per_image)))
    ctx = appCtx.Net.ctx
    E, status = ctx.embed_files([str(p) for p in paths], appCtx.Head, prec, threads)
    if (np.asarray(status) != _lib.ICL_OK).any():
        return (None, False) if dedupe_threshold is None else (None, False, [])
    lab = np.zeros((len(paths), len(labelSet)), np.float32)
    for i, labels in enumerate(labels_per_image):
        for col in LabelIndices(labels, labelSet):
            if 0 <= col < len(labelSet):
                lab[i, col] = 1.0  # GenerateLabelVector (embeddings.go:166-174)
    if state.ctx is None and state.engine is None:
        state.ctx = ctx
    if update is not None:
        state.update = int(update)
    if remove_ids is not None:
        state.remove(remove_ids)
    skipped = state.add(np.concatenate([E, lab], axis=1), list(ids), skip_duplicates=dedupe_threshold)  # CombineEmbeddings (:177-183)
    out = (state.as_map(), True) if state.recluster() else (None, False)
    return out if dedupe_threshold is None else out + (skipped,)
