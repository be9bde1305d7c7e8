"""The stages between the datasets of the reference's pipeline, on the device (graph_construction/data_transformer.py,
and the directory loops ``process()`` of preprocessing/point_cloud_builder.py:365-452 and
graph_construction/graph_builder.py:487-562).

The reference's stages hand their data on through directories of ``.pt`` files: point clouds, graphs, graphs cut by an
edge classifier, the input of the object-condensation stage.  ``DataTransformer`` applies a transform to every file of
a directory, ``ECCut`` / ``ECCutRefine`` are the transforms that cut a graph by the edge classifier's score, and
``build_point_clouds`` / ``build_graphs`` are the loops of the two builders.  All of them read with ``io.load_graph``
and write through ``io.GraphWriter`` in the format ``io`` documents (a ``torch.save`` of a plain dict, not a PyG
pickle), while the next events are built.

Out of scope: the Lightning checkpoint loaders (``ECFromChkpt``, ``MLGraphConstruction.from_chkpt``), the ``.pickle``
detector cache, worker processes (``max_processes`` and ``chunk_size`` are accepted and one process does the work).
"""

from __future__ import annotations

import json
import logging
import os
import random
from pathlib import Path

import torch
from torch import nn

from . import graph_cut
from .data import collate
from .hparams import HyperparametersMixin
from .io import GraphWriter, load_graph
from .point_cloud_builder import read_event

__all__ = ["DataTransformer", "ECCut", "ECCutRefine", "build_point_clouds", "build_graphs",
           "get_event_id_sector_from_str"]

logger = logging.getLogger(__name__)


def _default_device() -> torch.device:
    return torch.device("cuda" if torch.cuda.is_available() else "cpu")


def _plain(v):
    """hyperparameters as something YAML and JSON can hold"""
    if isinstance(v, dict):
        return {str(k): _plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    if isinstance(v, (bool, int, float, str)) or v is None:
        return v
    if torch.is_tensor(v) and v.numel() == 1:
        return v.item()
    return str(v)


class DataTransformer:
    def __init__(self, transform: nn.Module, *, device=None):
        """Applies a transformation function to all data files and saves them on disk.  ``device``: where the files
        are loaded to before the transform sees them (default: the GPU)."""
        self._transform = transform
        self._device = _default_device() if device is None else torch.device(device)

    def _apply(self, names, input_dir: Path, writer: GraphWriter) -> None:
        graphs = [load_graph(input_dir / n, self._device) for n in names]
        writer.write(self._transform(graphs[0] if len(graphs) == 1 else collate(graphs)), names=names)

    def process(self, filename: str, *, input_dir: os.PathLike | str, output_dir: os.PathLike | str,
                redo: bool = True) -> None:
        """Process single file"""
        input_dir, output_dir = Path(input_dir), Path(output_dir)
        output_dir.mkdir(parents=True, exist_ok=True)
        if not redo and (output_dir / filename).is_file():
            # (the files are pre-filtered, but several jobs with different batching may work on one directory)
            return
        with GraphWriter(output_dir, redo=redo) as writer:
            self._apply([filename], input_dir, writer)

    def _save_hparams(self, input_dir: Path, output_dir: Path) -> None:
        """Save hyperparameters to disk: the transform's plus ``input_dir``, as YAML (where ``yaml`` is missing as
        JSON, which is valid YAML)"""
        output_dir.mkdir(parents=True, exist_ok=True)
        hparams = _plain(dict(getattr(self._transform, "hparams", {})))
        hparams["input_dir"] = str(input_dir)
        try:
            import yaml
        except ImportError:
            text = json.dumps(hparams, indent=1)
        else:
            text = yaml.safe_dump(hparams)
        (output_dir / "hparams").write_text(text)

    def process_directories(self, input_dirs: list[os.PathLike | str], output_dirs: list[os.PathLike | str], *,
                            redo=True, max_processes=1, chunk_size=1, start=0, n_files=0, seed=None,
                            batch_size=1) -> None:
        """Process all files in the input directories and save them to the output directories.

        Args:
            input_dirs:
            output_dirs:
            redo: If True, overwrite existing files
            max_processes: accepted for compatibility: one process does the work
            chunk_size: accepted for compatibility
            start: Index of first file to process
            n_files: Number of files to process. If 0, process all files from `start` on
            seed: Seed for shuffling of input files (exactly ``random.seed(seed); random.shuffle(sorted names)``).
                If None, no shuffling.  Shuffling with `redo=False` can help to submit more worker jobs later on.
            batch_size: how many files are collated and transformed in one launch sequence.  Only valid for
                transforms that treat the events of a collated batch independently and hand back a collated batch
                (``ECCut``, ``ECCutRefine``; a model whose output for an event depends on the other events of the
                batch is not such a transform).  The written files are those of ``batch_size=1``.
        """
        input_dirs, output_dirs = [Path(p) for p in input_dirs], [Path(p) for p in output_dirs]
        if len(input_dirs) != len(output_dirs):
            raise ValueError("input_dirs and output_dirs must have the same length")
        batch_size = max(1, int(batch_size))
        for input_dir, output_dir in zip(input_dirs, output_dirs):
            self._save_hparams(input_dir, output_dir)
            names = {p.name for p in input_dir.glob("*.pt")}
            if not redo:
                existing = {p.name for p in output_dir.glob("*.pt")}
                assert existing.issubset(names)
                logger.info("Skipping %d existing files", len(existing))
                names = names - existing
            names = sorted(names)
            if seed is not None:
                random.seed(seed)
                random.shuffle(names)
            names = names[start:start + n_files if n_files > 0 else None]
            with GraphWriter(output_dir, redo=redo) as writer:
                for a in range(0, len(names), batch_size):
                    self._apply(names[a:a + batch_size], input_dir, writer)


def _save_sub_hyperparameters(self, key: str, obj) -> None:
    """utils/lightning.py:18-56: the hyperparameters of ``obj`` under ``key`` (a warning for an object without any)"""
    if not hasattr(obj, "hparams"):
        logger.warning("Can't save hyperparameters from object of type %s. Make sure to inherit from "
                       "HyperparametersMixin.", type(obj))
        return
    assert key not in self.hparams
    self.save_hyperparameters({key: {"class_path": obj.__class__.__module__ + "." + obj.__class__.__name__,
                                     "init_args": dict(obj.hparams)}})


class ECCut(nn.Module, HyperparametersMixin):
    # noinspection PyUnusedLocal
    def __init__(self, ec: nn.Module, thld: float):
        """Applies a cut to the edge classifier output and saves the trimmed down graphs: ``ec_score`` holds the
        score of the kept edges.  The comparison ``w > thld`` is strict and made in float32; an edge with a NaN score
        is kept in no graph.  One event or a collated batch (``batch`` and ``ptr`` stay as they are: no hit is
        dropped).  Mask and compaction are ``gnntrk_threshold_compact`` (one host read: the number of kept edges)."""
        super().__init__()
        self.save_hyperparameters(ignore=["ec"])
        _save_sub_hyperparameters(self, "ec", ec)
        self._model = ec

    def forward(self, data):
        w = self._model(data)["W"]
        data.ec_score = w
        return graph_cut.edge_cut(data, w, float(self.hparams.thld))[0]


class ECCutRefine(nn.Module, HyperparametersMixin):
    # noinspection PyUnusedLocal
    def __init__(self, thld: float, name="ec_score"):
        """Similar to `ECCut`, but assumes that the edge classifier output is in a field named ``name``"""
        super().__init__()
        self.save_hyperparameters()

    def forward(self, data):
        return graph_cut.edge_cut(data, data[self.hparams.name], float(self.hparams.thld))[0]


# ------------------------------------------------------------------------------------- the loops of the two builders
_HITS_SUFFIXES = ("-hits.csv.gz", "-hits.csv")


def build_point_clouds(builder, indir, outdir, *, start: int | None = None, stop: int | None = None, redo: bool = True,
                       ignore_loading_errors: bool = False) -> list[Path]:
    """``PointCloudBuilder.process``: every event ``<prefix>-{hits,cells,particles,truth}.csv[.gz]`` of ``indir`` (the
    prefixes in sorted order, ``[start:stop]`` of them) through ``read_event`` and ``builder.build(..., collated=True)``
    to one file ``data{evtid}_s{sector}.pt`` per sector in ``outdir``; ``evtid`` is the number in the last nine
    characters of the prefix.  ``redo=False`` leaves existing files alone (an event whose files all exist is not
    built).  ``builder.stats`` and ``builder.measurements`` are filled as ``build`` fills them.  Returns the written
    paths."""
    indir, outdir = Path(indir), Path(outdir)
    prefixes = []
    for p in sorted(indir.iterdir()):
        for suffix in _HITS_SUFFIXES:
            if p.name.endswith(suffix) and indir / p.name[:-len(suffix)] not in prefixes:
                prefixes.append(indir / p.name[:-len(suffix)])
    with GraphWriter(outdir, redo=redo) as writer:
        for prefix in prefixes[start:stop]:
            evtid = int(prefix.name[-9:])
            names = [f"data{evtid}_s{s}.pt" for s in range(builder.n_sectors)]
            if not redo and all((outdir / n).is_file() for n in names):
                logger.debug("skipping event %d", evtid)
                continue
            try:
                tables = read_event(prefix)
            except Exception:
                if ignore_loading_errors:
                    logger.exception("Error loading event %d", evtid)
                    continue
                raise
            writer.write(builder.build(tables, evtid, collated=True), names=names)
    return writer.written


def get_event_id_sector_from_str(name: str) -> tuple[int, int]:
    """``data{evtid}_s{sector}.pt`` -> (evtid, sector) (graph_construction/graph_builder.py:472-485)"""
    number_s = name.split(".")[0][len("data"):]
    evtid_s, sectorid_s = number_s.split("_s")
    return int(evtid_s), int(sectorid_s)


def build_graphs(builder, indir, outdir, *, start: int = 0, stop: int | None = 1, only_sector: int = -1,
                 redo: bool = True, batch_size: int = 1) -> list[Path]:
    """``GraphBuilder.process``: the point cloud files ``sorted(indir)[start:stop]`` (the reference's defaults: the
    first file only) that end in ``.pt`` through ``load_graph`` and ``builder.build`` to a graph file of the same name
    in ``outdir``.  A name that is not ``data{evtid}_s{sector}.pt`` raises ``ValueError("<name> is not a valid file
    name")``; ``only_sector >= 0`` keeps that sector only; ``redo=False`` skips files that exist in ``outdir``.
    ``batch_size`` clouds are collated and built in one launch sequence.  ``builder.measurements`` is filled as
    ``build`` fills it.  Returns the written paths."""
    indir, outdir = Path(indir), Path(outdir)
    dev = _default_device()
    todo = []
    for f in sorted(indir.iterdir())[start:stop]:
        if f.suffix != ".pt":
            continue
        try:
            evtid, sector = get_event_id_sector_from_str(f.name)
        except (ValueError, KeyError) as e:
            raise ValueError(f"{f.name} is not a valid file name") from e
        if 0 <= only_sector != sector:
            continue
        if not redo and (outdir / f.name).is_file():
            continue
        todo.append((f, evtid, sector))
    batch_size = max(1, int(batch_size))
    with GraphWriter(outdir, redo=redo) as writer:
        for a in range(0, len(todo), batch_size):
            part = todo[a:a + batch_size]
            clouds = [load_graph(f, dev) for f, _, _ in part]
            if len(part) == 1:
                graph = builder.build(clouds[0], evtid=part[0][1], s=part[0][2])
            else:
                graph = builder.build(collate(clouds))
                graph.evtid = torch.tensor([e for _, e, _ in part], dtype=torch.int64, device=graph.x.device)
                graph.s = torch.tensor([s for _, _, s in part], dtype=torch.int64, device=graph.x.device)
            writer.write(graph, names=[f.name for f, _, _ in part])
    return writer.written
