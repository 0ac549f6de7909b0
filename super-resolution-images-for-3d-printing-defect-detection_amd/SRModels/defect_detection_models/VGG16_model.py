"""Frozen-VGG16 defect classifier on MI355X behind the reference's class surface
(reference: defect_detection_models/VGG16_model.py).

Graph (VGG16_model.py:69-97): VGG16 conv base (13 x conv3x3+ReLU, 5 x maxpool) -> GAP -> Dense256 ReLU ->
Dense(num_classes) softmax; inputs are [0,1] floats with no ImageNet preprocessing; Dropout is identity at
inference.  ImageNet weights cannot be fetched offline: weights come from a checkpoint or a seeded init.
"""
import os

import numpy as np
import torch

from sr355 import pipeline as P
from sr355.wrappers import DeviceModelMixin, load_pretrained


class FineTunedVGG16(DeviceModelMixin):
    _init_scheme = "he_normal"

    def __init__(self, compute_dtype="f32"):
        self.model = None
        self.trained = False
        self.compute_dtype = compute_dtype
        self.input_shape = None

    def _mark_trained(self, v):
        self.trained = v

    def setup_model(self, input_shape=(128, 128, 3), num_classes=2, train_last_n_layers=4, base_trainable=False, dropout_rate=0.2,
                    l2_reg=0.0, learning_rate=1e-3, loss="sparse_categorical_crossentropy", from_pretrained=False,
                    pretrained_path=None, fine_tune_base=False):
        """VGG16_model.py:29-109.  fine_tune_base (not in the reference; default False = the reference's head-only training, whatever
        base_trainable says, see below): True makes `fit` train, with the two Dense layers and under the same Adam, the convs among the last
        `train_last_n_layers` of the base's 19 Keras layers (input_1, 13 convs, 5 pools in graph order: 4 -> block5_conv1..3, 6 -> those and
        block4_conv3, 1 -> none, i.e. head-only, >= 18 -> all 13; sr355.vgg_train.vgg16_tail_convs) -- what the reference's flags read like and
        never do.  `base_trainable` is not consulted by this flag."""
        assert input_shape[-1] == 3, "Input must have 3 channels (RGB)."
        self.input_shape = tuple(input_shape)
        weights = load_pretrained(pretrained_path) if from_pretrained else None
        if weights is not None:
            num_classes = int(weights["predictions"][0].shape[-1])
        # base_trainable / train_last_n_layers (VGG16_model.py:75-82): the reference sets `base.trainable = False` on the nested VGG16
        # model and then `layer.trainable = True` on its last n sub-layers.  In Keras a frozen parent model keeps its sub-layers' weights
        # out of trainable_weights whatever their own flag says, and the base is called with training=False: the base STAYS FROZEN, and
        # the notebook that passes (train_last_n_layers=6, base_trainable=True) reports 131 842 trainable parameters = the two Dense
        # layers (VGG16.ipynb:L152,L161-165).  So both arguments are accepted and recorded, and training is the
        # same head-only training in either case -- the reference's behaviour, not its apparent intent.
        self.base_trainable, self.train_last_n_layers = bool(base_trainable), int(train_last_n_layers)
        self.fine_tune_base = bool(fine_tune_base)
        self.dropout_rate, self.l2_reg, self.learning_rate = float(dropout_rate), float(l2_reg), float(learning_rate)
        if loss != "sparse_categorical_crossentropy":
            raise ValueError("only sparse_categorical_crossentropy (the reference's default, VGG16_model.py:29) is built")
        self._make("vgg16", self.compute_dtype, num_classes=num_classes)
        if weights is not None:
            self.set_weights(weights)
            print(f"Loaded pretrained model from {pretrained_path}")
        else:
            self._random_init(seed=4000)

    def _tail_convs(self):
        from sr355.vgg_train import vgg16_tail_convs
        return vgg16_tail_convs(self.train_last_n_layers) if getattr(self, "fine_tune_base", False) else []

    def trainable_layers(self):
        """Layers whose parameters `fit` updates: the two Dense layers, with or without base_trainable; with fine_tune_base the base's
        trainable convs in front of them (see setup_model)."""
        return self._tail_convs() + ["dense", "predictions"]

    def count_params(self, trainable_only=False):
        """Keras `model.count_params()` / the "Trainable params" line of model.summary(): 14 846 530 / 131 842 at num_classes=2
        (VGG16.ipynb:L151-153)."""
        names = self.trainable_layers() if trainable_only else list(self.weights)
        return int(sum(np.asarray(k).size + np.asarray(b).size for k, b in (self.weights[n] for n in names)))

    # ------------------------------------------------------------------ training of the head on the frozen base (VGG16_model.py:111-166)
    def _gap_device(self, x):
        """[n,H,W,3] device tensor (fp32, or the compute dtype) -> fp32 device [n,512]: the frozen conv base (tap after block5_conv3),
        max-pool and GAP kernels."""
        from sr355 import _lib as L
        _, taps = self.model.forward_with_taps(x, ["block5_conv3"])
        return self.ctx.spatial_op(L.SP_GAP, self.ctx.spatial_op(L.SP_MAXPOOL2, taps["block5_conv3"]))

    def _prefix_device(self, x, first_conv):
        """[n,H,W,3] device tensor (fp32, or the compute dtype) -> fp32 device [n,h,w,C]: the input of the base conv `first_conv`, from the
        frozen layers in front of it (one tapped forward of the inference model, a max-pool launch where a pool sits between)."""
        from sr355 import _lib as L
        from sr355.vgg_train import vgg16_prefix_tap
        tap, pooled = vgg16_prefix_tap(first_conv)
        if tap is None:
            return x.float()
        _, taps = self.model.forward_with_taps(x, [tap])
        return self.ctx.spatial_op(L.SP_MAXPOOL2, taps[tap]) if pooled else taps[tap]

    def _gap_features(self, images, batch_size=256):
        """[n,H,W,3] in [0,1] -> [n,512] host features (the host reference path of fit): _gap_device per chunk, downloaded."""
        out = []
        for i in range(0, len(images), batch_size):
            x = self.ctx.to_device(np.asarray(images[i:i + batch_size], np.float32),
                                   torch.bfloat16 if self.compute_dtype == "bf16" else torch.float32)
            out.append(self._gap_device(x).cpu().numpy().reshape(len(x), -1))
        return np.concatenate(out) if out else np.zeros((0, 512), np.float32)

    @staticmethod
    def _augment_params(rng, n, h, w, rotation_range=20, width_shift_range=0.2, height_shift_range=0.2, horizontal_flip=True):
        """The random draws of _augment for n images of h x w, in its order (per image: angle, ty, tx, then the flip's random()) ->
        (rot [n,2,2], offset [n,2], flip [n]): output pixel o samples input rot @ o + offset, then the columns are mirrored where flip."""
        rot, offset, flip = np.empty((n, 2, 2)), np.empty((n, 2)), np.zeros(n, bool)
        centre = np.array([(h - 1) / 2.0, (w - 1) / 2.0])
        for i in range(n):
            th = np.deg2rad(rng.uniform(-rotation_range, rotation_range))
            ty, tx = rng.uniform(-height_shift_range, height_shift_range) * h, rng.uniform(-width_shift_range, width_shift_range) * w
            c, s_ = np.cos(th), np.sin(th)
            rot[i] = np.array([[c, -s_], [s_, c]])
            offset[i] = centre - rot[i] @ centre + np.array([ty, tx])
            flip[i] = horizontal_flip and rng.random() < 0.5
        return rot, offset, flip

    @staticmethod
    def _augment(x, rng, rotation_range=20, width_shift_range=0.2, height_shift_range=0.2, horizontal_flip=True):
        """One draw of keras ImageDataGenerator(rotation_range=20, width_shift_range=0.2, height_shift_range=0.2,
        horizontal_flip=True) per image (VGG16_model.py:129-134): random rotation about the centre, random shifts as fractions of
        the size, fill_mode 'nearest', bilinear interpolation, random flip.  The host reference (NumPy / SciPy) of the device's
        sr_affine_warp, which fit runs on the same parameters (_augment_params)."""
        from scipy import ndimage
        out = np.empty_like(x)
        h, w = x.shape[1:3]
        rot, offset, flip = FineTunedVGG16._augment_params(rng, len(x), h, w, rotation_range, width_shift_range, height_shift_range, horizontal_flip)
        for i, img in enumerate(x):
            for ch in range(img.shape[2]):
                out[i, :, :, ch] = ndimage.affine_transform(img[:, :, ch], rot[i], offset=offset[i], order=1, mode="nearest")
            if flip[i]:
                out[i] = out[i, :, ::-1]
        return out

    def fit(self, X_train, y_train, X_val, y_val, batch_size=32, epochs=50, use_augmentation=True, seed=42):
        """FineTunedVGG16.fit (VGG16_model.py:111-157), every per-batch step on the device: the batch's gather and augmentation
        (sr_affine_warp), the frozen conv base, and the two Dense layers' step (sr_dense_head_step + DeviceAdam, sparse CCE, Dropout,
        EarlyStopping / ReduceLROnPlateau: train.fit_head_device).  X_train and X_val are uploaded once per fit as fp32: the device holds
        4 N_train H W 3 bytes of training images for the whole fit, and 4 N_val H W 3 bytes of validation images only while their GAP
        features (2 KiB per image, kept) are computed, once.  The random draws stay
        the host's, draw for draw those of the host path (_augment / fit_head): per epoch the permutation and the augmentation parameters on
        this generator, uploaded with the dropout masks in one copy.  The base is frozen with and without base_trainable, as in the reference
        (setup_model).  With augmentation the batches are 32 images, as the reference's datagen.flow(..., batch_size=32) hard-codes.
        X_train and / or X_val may be the X view of a sr355.patches.LabeledPatches (load_defects_dataset_as_patches(..., on_device=True)):
        then no fp32 patch array of that set exists anywhere -- each epoch's permutation goes up through set_order, a training batch is one
        sr_gather_warp_patches launch on the resident uint8 frames (the identity parameters without augmentation) and the validation
        features come from batch() chunks of 256 -- and the history and the head are, bit for bit, those of the equivalent arrays.
        With setup_model(fine_tune_base=True) and at least one conv among the last train_last_n_layers: the same fit, draws and callbacks over
        the trainable convs and the head together (sr355.vgg_train.VGGFineTuner: one flat bucket, one Adam; ReduceLROnPlateau acts on it and
        EarlyStopping restores convs and head of the best epoch; the host reads the whole bucket once per epoch for it).  Per batch the frozen
        prefix runs in the inference model and the trained tail in fp32; validation runs through the tail with the epoch's weights, from the
        validation set's frozen-prefix activations, which are computed once per fit and stay on the device as fp32 for the whole fit:
        4 h w C bytes per validation image at the first trained conv's input -- 128 KiB at train_last_n_layers=4 on 128 x 128 (8 x 8 x 512),
        512 KiB at 6 (16 x 16 x 512).  Afterwards set_weights carries the updated convs into the inference model."""
        from sr355.train import fit_head_device
        if self.model is None:
            raise ValueError("Model is not built yet.")
        from sr355.patches import labeled_dataset
        ds_train, ds_val = labeled_dataset(X_train), labeled_dataset(X_val)
        y_train, y_val = np.asarray(y_train, np.int64).reshape(-1), np.asarray(y_val, np.int64).reshape(-1)
        if ds_train is None:
            X_train = np.asarray(X_train, np.float32)
        if ds_val is None:
            X_val = np.asarray(X_val, np.float32)
        nc = int(np.asarray(self.weights["predictions"][0]).shape[-1])
        if len(y_train) != len(X_train) or (len(y_train) and (y_train.min() < 0 or y_train.max() >= nc)):
            raise ValueError(f"y_train: one label in [0, {nc}) per training image")
        rng = np.random.default_rng(seed)
        bs = 32 if use_augmentation else int(batch_size)
        n, (h, w) = len(X_train), X_train.shape[1:3]
        Xd = self.ctx.to_device(X_train) if ds_train is None else None
        convs, trainer = self._tail_convs(), None
        if convs:
            from sr355.vgg_train import VGGFineTuner
            trainer = VGGFineTuner(self.ctx, self.weights, convs, self.learning_rate)
        frozen = self._gap_device if trainer is None else (lambda x: self._prefix_device(x, convs[0]))
        if ds_val is None:
            Xv = self.ctx.to_device(X_val)
            g_val = [frozen(Xv[i:i + 256]) for i in range(0, len(X_val), 256)]
            del Xv
        else:
            ov = ds_val.set_order(np.arange(len(ds_val))) if len(ds_val) else None
            g_val = [frozen(ds_val.batch(ov, i, min(256, len(ds_val) - i))) for i in range(0, len(ds_val), 256)]
        if trainer is None:
            g_val = g_val[0] if len(g_val) == 1 else (torch.cat(g_val) if g_val else self.ctx.empty((0, 512)))
        else:
            p_val = g_val                                   # the cached prefix activations, in chunks of 256 images

            def g_val():
                g = [trainer.tail_features(p[i:i + bs]) for p in p_val for i in range(0, len(p), bs)]
                return g[0] if len(g) == 1 else torch.cat(g)
        epoch_order = {}

        def draw_epoch(epoch):
            order = rng.permutation(n)
            if use_augmentation:
                rot, off, flip = self._augment_params(rng, n, h, w)
            else:
                rot, off, flip = np.broadcast_to(np.eye(2), (n, 2, 2)), np.zeros((n, 2)), np.zeros(n, bool)
            plan = {"labels": y_train[order].astype(np.int32), "warp": self.ctx.warp_params(rot, off, flip)}
            if ds_train is None:
                plan["idx"] = order.astype(np.int32)
            else:
                epoch_order["dev"] = ds_train.set_order(order)          # validated on the host, as table rows
            return plan

        def features(dev, i, j):
            if ds_train is None:
                return frozen(self.ctx.affine_warp(Xd, dev["idx"][i:j], dev["warp"][i:j]))
            return frozen(ds_train.warped_batch(epoch_order["dev"], i, j - i, dev["warp"][i:j]))

        head, history = fit_head_device(self.ctx, features, self.weights, draw_epoch, n, g_val, y_val, learning_rate=self.learning_rate, batch_size=bs,
                                        epochs=epochs, dropout_rate=self.dropout_rate, l2_reg=self.l2_reg, seed=seed, trainer=trainer)
        w_ = dict(self.weights)
        w_.update(head)
        self.set_weights(w_)
        self.trained = True
        return history

    def evaluate(self, X_test, y_test):
        """model.evaluate -> [loss, accuracy] (VGG16_model.py:159-166)."""
        from sr355.train import sparse_cce
        if not self.trained:
            raise RuntimeError("Model has not been trained.")
        from sr355.patches import labeled_dataset
        p = np.asarray(self.predict(X_test if labeled_dataset(X_test) is not None else np.asarray(X_test, np.float32)), np.float64)
        loss, acc = sparse_cce(p, np.asarray(y_test, np.int64).reshape(-1))
        if self.l2_reg > 0:
            loss += self.l2_reg * float(np.sum(np.asarray(self.weights["dense"][0], np.float64) ** 2))
        print(f"Loss: {loss:.4f}, Accuracy: {acc:.4f}")
        return [loss, acc]

    def predict(self, patches, batch_size=32):
        """model.predict.  A view of a sr355.patches.LabeledPatches is gathered on the device in chunks that are multiples of batch_size, so
        every forward sees the patches it would see in the array, and gives the array's result."""
        from sr355.patches import labeled_dataset
        ds = labeled_dataset(patches)
        if ds is None:
            return self.model.predict(patches, batch_size=batch_size)
        bs = max(1, int(batch_size))
        chunk, n = bs * max(1, 4096 // bs), len(ds)
        if n == 0:
            return np.zeros((0, int(np.asarray(self.weights["predictions"][0]).shape[-1])), np.float32)
        order = ds.set_order(np.arange(n))
        return np.concatenate([self.model.predict(ds.batch(order, i, min(chunk, n - i)), batch_size=bs).float().cpu().numpy()
                               for i in range(0, n, chunk)])

    def classify_defects_method(self, image, patch_size=None, stride=None, batch_size=32):
        """Patch the image, classify every patch, majority vote (VGG16_model.py:168-270).
        Returns (predicted_class: int, confidence: float)."""
        if self.model is None:
            raise ValueError("Model is not built yet.")
        if image is None:
            raise ValueError("image must be provided")
        shape = tuple(image.shape)
        if len(shape) != 3 or shape[2] != 3:
            raise ValueError("image must be HxWx3 RGB array")
        if patch_size is None:
            if self.input_shape is None or self.input_shape[0] is None:
                raise ValueError("Model input size is dynamic; please set patch_size.")
            patch_size = int(self.input_shape[0])
        if stride is None:
            stride = max(1, patch_size // 2)
        img, _ = P.as_device_image(self.ctx, image)
        patches = self.ctx.extract_patches(img, patch_size, stride)
        probs = self.model.predict(patches, batch_size=max(int(batch_size), 128))
        return P.majority_vote(probs.float().cpu().numpy())

    # Bytes of fp32 patches one chunk of classify_defects_batch may hold.  Model.predict keeps its whole input and output resident and only
    # forwards `batch_size` patches at a time, so the patch tensor is the one allocation that grows with the number of frames; 1 GiB is
    # 9 709 patches of 96 x 96 x 3 fp32: 119 dataset frames (478 x 478, 81 patches) per chunk, and a single 1080p x4 frame (14 400 patches,
    # 1.5 GiB) is a chunk of its own -- a chunk is never less than one frame.
    patch_budget_bytes = 1 << 30

    def _frame_stack(self, images):
        """[F,H,W,3] ndarray / device tensor / list of equally sized images -> contiguous device stack, uint8 (values as they are) when every
        frame is uint8, else fp32 (`as_device_image`'s conversion per frame)."""
        ctx = self.ctx
        if images is None:
            raise ValueError("images must be provided")
        if isinstance(images, (list, tuple)):
            if not images:
                raise ValueError("images must hold at least one frame")
            shapes = {tuple(f.shape) for f in images}
            if len(shapes) != 1:
                raise ValueError(f"images must all have the same size, got {sorted(shapes)}")
            if any(len(s) != 3 or s[2] != 3 for s in shapes):
                raise ValueError("every image must be HxWx3 RGB array")
            if all(not isinstance(f, torch.Tensor) for f in images):
                images = np.stack([np.asarray(f) for f in images])
            else:
                return torch.stack([P.as_device_image(ctx, f)[0] for f in images])
        shape = tuple(images.shape)
        if len(shape) != 4 or shape[3] != 3 or shape[0] < 1:
            raise ValueError("images must be an [F,H,W,3] RGB stack")
        if isinstance(images, torch.Tensor):
            return images.to(ctx.torch_device, torch.uint8 if images.dtype == torch.uint8 else torch.float32).contiguous()
        a = np.asarray(images)
        return ctx.to_device(a if a.dtype == np.uint8 else a.astype(np.float32, copy=False))

    def classify_defects_batch(self, images, patch_size=None, stride=None, batch_size=32, raw=False):
        """classify_defects_method for F equally sized frames with one host read: one batched patch extraction, one predict over all F*P
        patches, one vote on the device (sr_patch_vote: the reference's rule, fp64 means), one read at the end.

        images: [F,H,W,3] ndarray (uint8 [0,255] or float), device tensor, or list of equally sized images (ValueError otherwise).  Defaults and
        exceptions are classify_defects_method's.  Returns (classes int64 [F], confidences float64 [F]); raw=True returns the int32 / fp32
        device tensors and reads nothing.  F is cut into chunks whose fp32 patch tensor stays within `patch_budget_bytes` (1 GiB: predict
        keeps its whole input resident, see the attribute), at least one frame per chunk; chunks change no frame's result."""
        if self.model is None:
            raise ValueError("Model is not built yet.")
        if patch_size is None:
            if self.input_shape is None or self.input_shape[0] is None:
                raise ValueError("Model input size is dynamic; please set patch_size.")
            patch_size = int(self.input_shape[0])
        if stride is None:
            stride = max(1, patch_size // 2)
        stack = self._frame_stack(images)
        F, H, W, _ = stack.shape
        per_frame = self.ctx.num_patches(H, W, 3, patch_size, stride)
        chunk = max(1, int(self.patch_budget_bytes) // max(1, per_frame * patch_size * patch_size * 3 * 4))
        cls, conf = [], []
        for i in range(0, F, chunk):
            patches = self.ctx.extract_patches_batch(stack[i:i + chunk], patch_size, stride)
            probs = self.model.predict(patches, batch_size=max(int(batch_size), 128))
            c, p, _ = self.ctx.patch_vote(probs, len(stack[i:i + chunk]), per_frame, raw=True)
            cls.append(c)
            conf.append(p)
        cls, conf = (cls[0], conf[0]) if len(cls) == 1 else (torch.cat(cls), torch.cat(conf))
        if raw:
            return cls, conf
        both = torch.stack([cls.to(torch.float32), conf]).cpu().numpy()              # a class index is exact in fp32: one read for both
        return both[0].astype(np.int64), both[1].astype(np.float64)

    def save(self, directory, timestamp, fmt="npz"):
        """VGG16_model.py:272-283; fmt="h5" writes Keras' weight layout (sr355.h5lite), "npz" this build's container."""
        if not self.trained:
            raise RuntimeError("Cannot save an untrained model.")
        path = self._save_weights(directory, f"VGG16_{timestamp}", fmt)
        print(f"Model saved to {path}")
        return path
