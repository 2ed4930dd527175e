"""Dataset validation: CRC-verify every frame of a TFRecord dataset.

The reference has no fsck equivalent — corruption only surfaces when a read
hits it. This walks every data file, discovers frame boundaries (GPU
parallel scan when available) and checks both masked CRC32Cs of every
record, returning a per-file report without decoding any payloads.
"""

from __future__ import annotations

import os
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

from .. import _native
from .. import engine as engine_mod
from . import paths as P

__all__ = ["validate_tfrecord", "FileReport", "ValidationReport"]


@dataclass
class FileReport:
    path: str
    records: int
    bytes: int
    ok: bool
    error: Optional[str] = None


@dataclass
class ValidationReport:
    files: List[FileReport] = field(default_factory=list)

    @property
    def ok(self) -> bool:
        return all(f.ok for f in self.files)

    @property
    def records(self) -> int:
        return sum(f.records for f in self.files)

    def __repr__(self):
        bad = [f.path for f in self.files if not f.ok]
        return (f"ValidationReport(files={len(self.files)}, "
                f"records={self.records}, ok={self.ok}"
                + (f", bad={bad}" if bad else "") + ")")


def _validate_one(fpath: str, eng: str) -> FileReport:
    size = os.path.getsize(fpath)
    try:
        if eng == "gpu" and size:
            from ..engine import gpu as gpu_engine

            # None (a file for the host codec: foreign gzip, deflate,
            # TFREC_SNAPPY=host, or one the device refused) drops through
            # to the host path
            data = gpu_engine.read_file_image(fpath)
            if data is not None:
                if data.numel() == 0:
                    return FileReport(fpath, 0, size, True)
                off, lens = gpu_engine.scan_frames_device(data)
                gpu_engine.crc_verify_device(data, off, lens)
                return FileReport(fpath, int(off.numel()), size, True)
        raw = np.frombuffer(P.decompress_file(fpath), np.uint8)
        if raw.size == 0:
            return FileReport(fpath, 0, size, True)
        off, _ = _native.scan_frames(raw, True)  # verifies CRCs on host
        return FileReport(fpath, len(off), size, True)
    except Exception as e:  # noqa: BLE001 — report, don't raise
        return FileReport(fpath, 0, size, False, str(e))


def validate_tfrecord(path: str, engine: str = "auto") -> ValidationReport:
    files = P.list_data_files(path)
    if not files:
        raise FileNotFoundError(f"No TFRecord files found under {path}")
    eng = engine_mod.resolve_engine(engine)
    rep = ValidationReport()
    for f in files:
        rep.files.append(_validate_one(f, eng))
    return rep
