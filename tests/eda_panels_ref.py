"""NumPy restatement of the EDA's per-pair panels (reference data/EDA.ipynb, cell 769cc582: save_visual_example,
create_advanced_visualizations, create_global_advanced_visualizations), the contract of sr_eda_pair_panels and of
data/eda_methods.py's ImageDataVisualization.  Written from the reference cell's expressions on top of tests/eda_ref.py's 8-bit
planes (gray, blur5, HSV: restated from OpenCV's documented behaviour there, not pinned against cv2), not from the device code.

  spectrum   np.abs(np.fft.fftshift(np.fft.fft2(gray))); the panel shows np.log(mag + 1e-8)
  gradient   sqrt(sobelx^2 + sobely^2) of cv2.Sobel(gray_hr, CV_64F, ksize=5)
  GLCM       graycomatrix(lr_gray, [1], [0], 256, symmetric=True, normed=True): (C + C^T) / sum, in fp64; graycoprops contrast
  noise map  np.mean(np.abs(lr - GaussianBlur(lr, (5, 5), 0)), axis=2): three integers summed, one division by 3; its mean over the
             image is the mean over all three channels, sum / (3 H W)
  saturation plt.hist(S.ravel(), bins=50, density=True): np.histogram over the plane's own [min, max]
  difference cvtColor(absdiff(lr, hr), BGR2GRAY); convertScaleAbs of a uint8 image and a resize to the same size change nothing"""
import numpy as np

from eda_ref import blur5_u8, fft_mag, glcm_counts, glcm_normed, glcm_props, grad5_mag, gray_u8, hsv_sv

EPS = 1e-8


def sat_density(s_plane):
    return np.histogram(np.asarray(s_plane).ravel(), bins=50, density=True)


def pair_panels(lr, hr):
    """Every output of sr_eda_pair_panels for one aligned BGR pair, plus the integer pieces the tests compare through."""
    lr, hr = np.asarray(lr), np.asarray(hr)
    gl, gh = gray_u8(lr), gray_u8(hr)
    counts = glcm_counts(gl, 256, (0,))[0]
    sym = counts + counts.T
    glcm = glcm_normed(counts)
    cn = np.abs(lr.astype(np.int64) - blur5_u8(lr).astype(np.int64))                 # exact integers
    noise = np.mean(cn.astype(np.float64), axis=2)
    s_lr, s_hr = hsv_sv(lr)[0], hsv_sv(hr)[0]
    absdiff = np.abs(lr.astype(np.int64) - hr.astype(np.int64)).astype(np.uint8)
    return {"spec_lr": fft_mag(gl), "spec_hr": fft_mag(gh), "grad_hr": grad5_mag(gh), "glcm_lr": glcm, "glcm_sym_counts": sym, "glcm_total": int(sym.sum()),
            "glcm_contrast": glcm_props(glcm)[0], "noise_lr": noise, "noise_sum": int(cn.sum()), "noise_mean": int(cn.sum()) / (3.0 * lr.shape[0] * lr.shape[1]),
            "diff": gray_u8(absdiff), "sat_hist": np.stack([np.bincount(s.ravel(), minlength=256) for s in (s_lr, s_hr)]).astype(np.int64),
            "sat_planes": (s_lr, s_hr), "gray_sum": (int(gl.astype(np.int64).sum()), int(gh.astype(np.int64).sum()))}


def advanced_panel(lr, hr):
    """create_advanced_visualizations' numbers under ImageDataVisualization.advanced_panel's names."""
    p = pair_panels(lr, hr)
    return {"lr_log_spectrum": np.log(p["spec_lr"] + EPS), "hr_log_spectrum": np.log(p["spec_hr"] + EPS), "gradient_magnitude": p["grad_hr"],
            "lr_glcm": p["glcm_lr"], "lr_glcm_contrast": p["glcm_contrast"], "noise_map": p["noise_lr"], "color_noise_mean": p["noise_mean"],
            "sat_lr": sat_density(p["sat_planes"][0]), "sat_hr": sat_density(p["sat_planes"][1])}


def visual_example(lr, hr):
    lr, hr = np.asarray(lr), np.asarray(hr)
    return {"lr_rgb": lr[..., ::-1], "hr_rgb": hr[..., ::-1], "diff_gray": pair_panels(lr, hr)["diff"]}


def spectrum_floor(shape, gray_sum):
    """A-priori absolute error bound of one DFT bin formed as two chained dot products with unit-modulus factors in fp64:
    (H + W) 2^-52 sum(gray).  A bin near zero has no meaningful relative bound."""
    return (shape[0] + shape[1]) * 2.0 ** -52 * gray_sum


def global_advanced_panel(global_data):
    """create_global_advanced_visualizations' numbers; None where the reference prints and returns."""
    if global_data is None or global_data.get("count", 0) == 0:
        return None
    n = global_data["count"]
    out = {"lr_fft_avg": global_data["lr_fft_sum"] / n, "hr_fft_avg": global_data["hr_fft_sum"] / n, "grad_hr_avg": global_data["grad_hr_sum"] / n}
    out["lr_log_spectrum"], out["hr_log_spectrum"] = np.log(out["lr_fft_avg"] + EPS), np.log(out["hr_fft_avg"] + EPS)
    g = global_data["glcm_sum"]
    g = (g / g.sum())[:, :, 0, 0]
    out["glcm_avg"], out["glcm_contrast"] = g, glcm_props(g)[0]
    bins = global_data["sat_bins"]
    w = bins[1] - bins[0]
    out["sat_lr_density"] = global_data["sat_lr_counts"] / (global_data["sat_lr_counts"].sum() * w + EPS)
    out["sat_hr_density"] = global_data["sat_hr_counts"] / (global_data["sat_hr_counts"].sum() * w + EPS)
    out["sat_centers"] = 0.5 * (bins[:-1] + bins[1:])
    noise = np.array(global_data["noise_means_lr"], dtype=np.float64)
    out["noise_means"], out["noise_mean"], out["noise_std"] = noise, noise.mean(), noise.std()
    return out


def example_names(label, rank, rel_path):
    """run_eda_pipeline's output stems for one example: (parent, basic stem, advanced stem)."""
    import os
    rel_no_ext = os.path.splitext(rel_path.replace("\\", "/"))[0]
    parent, stem = os.path.dirname(rel_no_ext), os.path.basename(rel_no_ext)
    return parent, f"{label}_{rank}_{stem}", f"{label}_{rank}_advanced_{stem}"
