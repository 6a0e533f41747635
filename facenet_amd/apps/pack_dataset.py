# coding:utf-8
"""Decode a data set once: ``python -m facenet_amd.apps.pack_dataset <config>`` builds the decoded-pixel pack of
``dataset.path`` in ``dataset.resident_cache``, which training with ``dataset.resident: true`` then
loads into device memory instead of decoding the files every epoch.  Host only: no GPU is touched.  A pack that is still
valid for the data set is left alone."""
from __future__ import annotations

import time
from pathlib import Path

import click

from facenet_amd import config as config_mod


@click.command()
@click.argument("config", type=Path)
@click.option("--workers", default=8, type=int, help="Decode threads.")
def main(config, workers):
    from facenet_amd import dataset, resident
    cfg = config_mod.load_config(config)
    if not cfg.dataset.path:
        raise click.UsageError("the config names no dataset.path")
    if not cfg.dataset.resident_cache:
        raise click.UsageError("the config names no dataset.resident_cache to write the pack to")
    cache = Path(cfg.dataset.resident_cache).expanduser()
    dbase = dataset.Database(cfg.dataset)
    t0 = time.perf_counter()
    pack, hit = resident.ensure_pack(dbase, cache, workers=workers, log=print)
    dt = time.perf_counter() - t0
    print(f"{cache}: {pack.nrof_images} images, {pack.nbytes} bytes ({pack.nbytes / 2 ** 30:.3f} GiB), "
          f"{'already valid, checked' if hit else 'built'} in {dt:.1f} s")


if __name__ == "__main__":
    main()
