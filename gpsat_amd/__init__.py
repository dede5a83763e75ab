"""gpsat_amd -- MI355X-native local-expert exact-GP backend (drop-in for GPSat's model backend).

Only what the hot path needs lives here:
  csrc/       gfx950 HIP kernels + the C ABI (libgpsat_hip.so, declared in include/gpsat_hip.h)
  _lib.py     ctypes binding
  engine.py   packed-ragged batch API (fit + objective + predict for thousands of tiles per launch)
  models.py   HipGPRModel: per-tile class with the reference's BaseGPRModel interface
  dataprep.py DataPrep.bin_data / bin_data_by: raw observations -> binned table (gpsat_bin_batch);
              DataPrep.assign_tracks: lon, lat, datetime -> t, x, y, dr, dt, track
  prep.py     WGS84toEASE2 / EASE2toWGS84, diff_distance, guess_track_num, track_num_for_date (gpsat_project_batch,
              gpsat_track_batch)
"""
__all__ = ["Engine", "default_engine", "HipGPRModel", "get_model", "DataPrep"]


def __getattr__(name):
    if name in ("Engine", "default_engine", "BatchResult", "GpsatError"):
        from . import engine
        return getattr(engine, name)
    if name in ("HipGPRModel", "get_model"):
        from . import models
        return getattr(models, name)
    if name == "DataPrep":
        from . import dataprep
        return dataprep.DataPrep
    raise AttributeError(name)
