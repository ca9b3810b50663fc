"""What the tests of the anomaly-map scores share (metrics.score_maps, anomaly_metrics*, the detection records): the key sets the
results are pinned to, the bit comparison and the tiny model the detection sweeps run.  Plain helpers, imported by name; torch and
the model are imported only by the functions that need them, so the CPU tests can use the rest."""
import numpy as np

DEV = "cuda:0"
PARENT_METRIC_KEYS = {"dice", "precision", "recall", "FPR", "IoU", "mse", "PSNR", "AUC", "AUC_status", "AP", "best_dice", "best_threshold",
                      "SSIM", "maps"}
PP_METRIC_KEYS = {"dice_pp", "precision_pp", "recall_pp", "AUC_pp", "AUC_pp_status", "AP_pp", "best_dice_pp", "best_threshold_pp"}
PARENT_RECORD_KEYS = {"t_distance", "output", "mean", "mse", "threshold", "counts", "auc", "auc_status", "ap", "best_dice",
                      "best_threshold", "ssim"}
PP_RECORD_KEYS = {"sqerr_pp", "auc_pp", "ap_pp", "best_dice_pp", "best_threshold_pp"}


def host(t):
    return t.detach().cpu().numpy()


def bits(a, b):
    """The same dtype, shape and bits."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def bits_any_nan(a, b):
    """`bits`, with every fp64 NaN counting as the same NaN (a square root and a constant give different ones)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype == np.float64 and b.dtype == np.float64:
        a, b = np.where(np.isnan(a), np.nan, a), np.where(np.isnan(b), np.nan, b)
    return bits(a, b)


def tiny(size=32):
    """(GaussianDiffusion module, a small deterministic UNet on the device, a 200-step diffusion) for `size` x `size` images."""
    import GaussianDiffusion as GD
    from UNet import UNetModel
    from oracle import unet_oracle as uo
    m = UNetModel(img_size=size, base_channels=32, n_heads=2, attention_resolutions="16,8")
    m.load_state_dict(uo.fill_deterministic({k: tuple(v.shape) for k, v in m.state_dict().items()}))
    m.to(DEV).eval()
    d = GD.GaussianDiffusionModel([size, size], GD.get_beta_schedule(200, "linear"), noise="gauss")
    return GD, m, d
