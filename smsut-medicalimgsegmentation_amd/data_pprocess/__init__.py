"""Dataset preparation (the reference's data_pprocess/): raw volume -> resampled, cropped, windowed 8-bit slices, on the device."""
from .volume import (ResamplePlan, chaos_label_lut, prepare_volume, resample_plan, restore_labels, window_bounds,  # noqa: F401
                     write_slices)
