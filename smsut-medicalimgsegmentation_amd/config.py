"""Module-level constants mirroring the reference's ``config.py:7-95`` (the whole flag system there).

Dataset paths are not reproduced (the reference ships ``***`` placeholders); everything on the hot path is.
"""
from enum import Enum


class Modality(Enum):          # config.py:7-11
    ct = 0
    t1in = 1
    t1out = 2
    t2 = 3


seed = 2020                    # config.py:23
n_modal = len(Modality.__members__)
n_label = 4                    # config.py:26 (CHAOS: 4 organs + background)

num_iter_per_epoch = 150       # config.py:29
max_epoch = 200
exp_alpha = 1.0
weight_dc = 0.5                # config.py:32-33
weight_ce = 0.5

img_channels = 1
base_width = 16
input_size = 256               # config.py:50
batch_size = 8                 # config.py:56
num_workers = 6

lr = 1e-2                      # config.py:73-74
weight_decay = 1e-3
nce_layers = [5]               # config.py:77

# CoraNet (config.py:80-94).  The reference ships two-class weight vectors with the CHAOS values in comments ([1, 5, 5, 5, 5] /
# [5, 1, 1, 1, 1]); here they are (background, foreground) pairs, expanded to n_label + 1 entries when the trainer is built.
thres = 0.5
default_w = (1.0, 1.0)
w_con = (1.0, 5.0)
w_rad = (5.0, 1.0)
pre_epoch = 100
cora_epoch = 200
pred_step = 10


def class_weights(pair, labels=None):
    """``[background] + [foreground] * labels``: a (background, foreground) weight pair as the per-class vector of
    ``nn.CrossEntropyLoss(weight=...)``; ``labels`` defaults to the current ``n_label`` (read at call time: tests change it)."""
    return [float(pair[0])] + [float(pair[1])] * (n_label if labels is None else labels)

expr_root = "smsut_out"        # the reference's placeholder is '***/bimod-out' (config.py:46)
base_root = None               # processed PNG dataset root ('***/bimod' upstream, config.py:44); None -> synthetic slices
split_yaml = "semi-1910.yaml"  # config.py:54
test_hausdorff = False         # -p test also writes {modality}_hd_matrix.csv (Hausdorff and HD95; commented out upstream)
test_spacing = None            # voxel spacing of the -p test surface distances: None (voxels), one (sz, sy, sx) for every volume,
                               # or a mapping {volume key such as 'ct_001', or modality name such as 'ct': (sz, sy, sx)}
validate_on_device = False     # validation and -p test without the host in the loop: argmax + Dice overlap counts in one launch per
                               # batch, nothing read back before the loader is exhausted (csrc/evaluate.hip; same Dice, meter and files)
test_translation = False       # ugan trainers: -p test also writes {modality}_translation_matrix.csv (SSIM / PSNR / MAE of the translator's
                               # cycle x -> G(x, i->j) -> G(., j->i) and of its paired translations; csrc/similarity.hip, nothing read back
                               # before the loader is exhausted)
test_translation_pairs = (('t1in', 't1out'),)   # modality-name pairs whose slices a_pid_z / b_pid_z show the same anatomy (CHAOS t1in /
                               # t1out are registered acquisitions); a pair whose modalities or slices are not in the test set adds nothing
test_calibration = False       # -p test also writes {modality}_calibration.csv (reliability table, ECE / MCE / NLL / Brier / accuracy per
                               # modality at T = 1 and at the temperature fitted on the test loader) and temperature.txt
                               # (csrc/calibration.hip: one pass per batch, the batches' logits stay on the device for the fit)
test_calibration_bins = 15     # confidence bins of equal width, 1 .. 64
data_aug = dict(               # config.py:60-71
    rotate=True, rotate_degrees=15,
    resizeCrop=True, resizeCrop_size=input_size,
    elasticDeform=True, elasticDeform_sigmas=(9., 13.), elasticDeform_points=3,
    colorJitter=False, gammaCorrect=False, gammaCorrect_gammas=(0.7, 1.5),
)
