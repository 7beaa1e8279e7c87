"""cv2_hip.py — the cv2 calls on the reference's hot path, with OpenCV's names, signatures and array
conventions, executed by the HIP kernels of libofk.so.  `import cv2_hip as cv2` in the reference's scripts
covers: cvtColor(COLOR_BGR2GRAY), warpPerspective(INTER_LINEAR), goodFeaturesToTrack, calcOpticalFlowPyrLK, KalmanFilter, TERM_CRITERIA_*; undistortPoints and
fisheye.undistortPoints / distortPoints belong to the camera model (ofk.h: ofk_set_camera), which the reference does not have.

Reference call sites: of_module.py:40,44,63-76,80,86,88,122,152; velocity_measurment_node:113,120,133,163;
homography_experiments/homography.py (warpPerspective);
evaluate_exp.py:65,66,85,98,106; of_library.py:236,238,248,249.
Semantics are those of oracle/image_oracle.c (OpenCV's published algorithms with exact integer window sums).
"""
import numpy as np

try:
    from . import ofk
except ImportError:
    import ofk

COLOR_BGR2GRAY = 6
TERM_CRITERIA_COUNT = 1
TERM_CRITERIA_MAX_ITER = 1
TERM_CRITERIA_EPS = 2
OPTFLOW_USE_INITIAL_FLOW = 4
OPTFLOW_LK_GET_MIN_EIGENVALS = 8


def cvtColor(src, code):
    if code != COLOR_BGR2GRAY:
        raise NotImplementedError("only COLOR_BGR2GRAY is on the hot path")
    src = np.asarray(src)
    if src.ndim != 3 or src.shape[2] != 3 or src.dtype != np.uint8:
        raise ValueError("cvtColor(BGR2GRAY) expects an HxWx3 uint8 image")
    h, w = src.shape[:2]
    return ofk.default_context(w, h).gray_bgr8(src)


INTER_NEAREST, INTER_LINEAR, INTER_CUBIC, INTER_AREA, INTER_LANCZOS4 = 0, 1, 2, 3, 4
WARP_INVERSE_MAP = 16
BORDER_CONSTANT, BORDER_REPLICATE = 0, 1


def warpPerspective(src, M, dsize, dst=None, flags=INTER_LINEAR, borderMode=BORDER_CONSTANT, borderValue=0):
    """cv2.warpPerspective for HxW or HxWx3 uint8 images, INTER_LINEAR only (cv2's 5-bit fixed-point arithmetic; ofk.h:
    ofk_warp_perspective states the rule and where the evaluation of the coordinates differs from cv2's).  M maps the source to the
    destination and is inverted here in float64, unless flags carries WARP_INVERSE_MAP; dsize = (width, height).  borderMode:
    BORDER_CONSTANT or BORDER_REPLICATE; borderValue: one number 0..255 for every channel (or a sequence of equal numbers)."""
    flags = int(flags)
    if flags & ~WARP_INVERSE_MAP != INTER_LINEAR:
        raise NotImplementedError("warpPerspective: INTER_LINEAR only (other interpolations are out of scope)")
    if borderMode not in (BORDER_CONSTANT, BORDER_REPLICATE):
        raise NotImplementedError("warpPerspective: BORDER_CONSTANT and BORDER_REPLICATE only")
    src = np.asarray(src)
    if src.dtype != np.uint8 or not (src.ndim == 2 or (src.ndim == 3 and src.shape[2] in (1, 3))) or 0 in src.shape:
        raise ValueError("warpPerspective expects an HxW, HxWx1 or HxWx3 uint8 image")
    M = np.asarray(M, np.float64)
    if M.shape != (3, 3):
        raise ValueError("warpPerspective: M must be 3x3")
    bv = np.unique(np.asarray(borderValue, np.float64).reshape(-1)[:max(1, src.shape[2] if src.ndim == 3 else 1)])
    if len(bv) != 1 or bv[0] != int(bv[0]) or not 0 <= bv[0] <= 255:
        raise NotImplementedError("warpPerspective: borderValue is one integer 0..255 for every channel")
    if not flags & WARP_INVERSE_MAP:
        try:
            M = np.linalg.inv(M)
        except np.linalg.LinAlgError:
            raise ValueError("warpPerspective: M is singular") from None
    w, h = int(dsize[0]), int(dsize[1])
    ctx = ofk.default_context(max(w, src.shape[1]), max(h, src.shape[0]))
    return ctx.warp_perspective(src, M, (h, w), borderMode, int(bv[0]))[0]


IMREAD_UNCHANGED, IMREAD_GRAYSCALE, IMREAD_COLOR = -1, 0, 1


def imdecode(buf, flags=IMREAD_COLOR):
    """cv2.imdecode for baseline JPEG streams (what cv_bridge.compressed_imgmsg_to_cv2 calls for the reference's CompressedImage
    callback, velocity_measurment_node.py:112), decoded on the GPU.  IMREAD_COLOR: HxWx3 BGR; IMREAD_UNCHANGED: HxW for gray
    streams, HxWx3 otherwise.  Returns None - like OpenCV - if the buffer is not a stream the decoder supports."""
    if flags not in (IMREAD_COLOR, IMREAD_UNCHANGED):
        raise NotImplementedError("imdecode: IMREAD_COLOR and IMREAD_UNCHANGED only (gray conversion is cvtColor's job on this path)")
    data = np.asarray(buf, dtype=np.uint8).tobytes() if not isinstance(buf, (bytes, bytearray, memoryview)) else bytes(buf)
    try:
        h, w, ncomp = ofk.jpeg_info(data)
        if h > ofk.MAX_DIM or w > ofk.MAX_DIM:      # a corrupt SOF header can claim 65535 x 65535: not a frame, no context for it
            return None
        img = ofk.default_context(w, h).jpeg_decode([data])[0]
    except ofk.OfkError:                            # unsupported / truncated stream, or no memory for a frame this size
        return None
    return np.ascontiguousarray(img[:, :, 0]) if (ncomp == 1 and flags == IMREAD_UNCHANGED) else img


def goodFeaturesToTrack(image, maxCorners, qualityLevel, minDistance, corners=None, mask=None, blockSize=3,
                        useHarrisDetector=False, k=0.04):
    if useHarrisDetector:
        raise NotImplementedError("the reference only uses the min-eigenvalue (Shi-Tomasi) detector")
    image = np.asarray(image)
    if image.ndim != 2 or image.dtype != np.uint8:
        raise ValueError("goodFeaturesToTrack expects an HxW uint8 image")
    h, w = image.shape
    if maxCorners <= 0:
        maxCorners = 4096
    ctx = ofk.default_context(w, h, min_pts=int(maxCorners))
    pts = ctx.good_features(image, int(maxCorners), float(qualityLevel), float(minDistance), int(blockSize), mask=mask)
    return pts if len(pts) else None           # OpenCV's Python binding returns None when nothing is found


def _criteria(criteria):
    typ, cnt, eps = criteria
    if not typ & TERM_CRITERIA_COUNT:
        cnt = 30
    if not typ & TERM_CRITERIA_EPS:
        eps = 0.01
    return int(cnt), float(eps)


def calcOpticalFlowPyrLK(prevImg, nextImg, prevPts, nextPts=None, status=None, err=None, winSize=(21, 21), maxLevel=3,
                         criteria=(TERM_CRITERIA_COUNT | TERM_CRITERIA_EPS, 30, 0.01), flags=0, minEigThreshold=1e-4):
    """flags: OPTFLOW_USE_INITIAL_FLOW (nextPts holds the start positions; ofk.h: at the top pyramid level) and
    OPTFLOW_LK_GET_MIN_EIGENVALS (err = minimum eigenvalue of the level-0 normal matrix per window pixel)."""
    flags = int(flags)
    if flags & ~(OPTFLOW_USE_INITIAL_FLOW | OPTFLOW_LK_GET_MIN_EIGENVALS):
        raise ValueError(f"calcOpticalFlowPyrLK: unknown flag bits {flags:#x}")
    if winSize[0] != winSize[1]:
        raise NotImplementedError("square windows only (the reference uses (15,15))")
    prevImg = np.asarray(prevImg); nextImg = np.asarray(nextImg)
    if prevImg.ndim != 2 or prevImg.dtype != np.uint8 or nextImg.shape != prevImg.shape or nextImg.dtype != np.uint8:
        raise ValueError("calcOpticalFlowPyrLK expects two HxW uint8 images of equal size")
    h, w = prevImg.shape
    pts = np.asarray(prevPts, np.float32).reshape(-1, 2)
    init = None
    if flags & OPTFLOW_USE_INITIAL_FLOW:
        if nextPts is None:
            raise ValueError("calcOpticalFlowPyrLK: OPTFLOW_USE_INITIAL_FLOW needs nextPts")
        init = np.asarray(nextPts, np.float32).reshape(-1, 2)
        if len(init) != len(pts):                       # OpenCV asserts nextPts.checkVector(2) == npoints
            raise ValueError(f"calcOpticalFlowPyrLK: nextPts has {len(init)} points, prevPts {len(pts)}")
        if not np.all(np.abs(init) <= 1e6):
            raise ValueError("calcOpticalFlowPyrLK: nextPts must be finite coordinates within 1e6")
    cnt, eps = _criteria(criteria)
    ctx = ofk.default_context(w, h, min_pts=max(1, len(pts)), min_level=int(maxLevel))
    return ctx.lk_pyr(prevImg, nextImg, pts, win=int(winSize[0]), max_level=int(maxLevel), max_count=cnt, eps=eps,
                      min_eig_thr=float(minEigThreshold), next_pts=init, flags=flags)


def _camera_matrix(m, what):
    m = np.asarray(m, np.float64)
    if m.ndim != 2 or m.shape[0] != 3 or m.shape[1] not in (3, 4):
        raise ValueError(f"{what} must be 3x3 (P: or 3x4)")
    if m[0, 1] != 0.0:
        raise NotImplementedError(f"{what}: no skew term")
    return float(m[0, 0]), float(m[1, 1]), float(m[0, 2]), float(m[1, 2])


def _points_32fc2(src, who):
    src = np.asarray(src)
    if src.dtype != np.float32:
        raise ValueError(f"{who}: CV_32FC2 points only (got {src.dtype})")
    if src.size % 2 or src.shape[-1] != 2:
        raise ValueError(f"{who}: points must be (N,1,2) or (N,2)")
    return src, np.ascontiguousarray(src.reshape(-1, 2))


def _identity_only(R, who):
    if R is not None and not np.array_equal(np.asarray(R, np.float64), np.eye(3)):
        raise NotImplementedError(f"{who}: a rectification R other than the identity is not supported")


def _lens_points(who, distort, model, src, K, k, P, iters):
    src, pts = _points_32fc2(src, who)
    fx, fy, cx, cy = _camera_matrix(K, "cameraMatrix")
    fo_x, fo_y, co_x, co_y = (1.0, 1.0, 0.0, 0.0) if P is None else _camera_matrix(P, "P")
    cam = ofk.camera_setting(model, fx, fy, cx, cy, k, iters, fo_x, fo_y, co_x, co_y)
    if not len(pts):
        return src.copy()
    ctx = ofk.default_context()
    out = (ctx.distort_points if distort else ctx.undistort_points)(cam, pts)
    return out.reshape(src.shape)


def undistortPoints(src, cameraMatrix, distCoeffs, R=None, P=None, criteria=None):
    """cv2.undistortPoints / undistortPointsIter for CV_32FC2 points ((N,1,2) or (N,2) float32; float64 raises): 4, 5 or 8 distortion
    coefficients (k1 k2 p1 p2 [k3 [k4 k5 k6]]), no R other than the identity, P None = normalised output.  The fixed-point count is
    cv2's 5 unless `criteria` carries TERM_CRITERIA_COUNT; it is a FIXED count (an EPS in the criteria is not looked at), see
    ofk.camera_setting for what 5 leaves on a wide-angle lens."""
    _identity_only(R, "undistortPoints")
    k = [] if distCoeffs is None else np.asarray(distCoeffs, np.float64).reshape(-1)
    if len(k) not in (0, 4, 5, 8):
        raise ValueError(f"undistortPoints: {len(k)} distortion coefficients (4, 5 or 8 are supported)")
    iters = 5
    if criteria is not None and int(criteria[0]) & TERM_CRITERIA_COUNT:
        iters = int(criteria[1])
    return _lens_points("undistortPoints", False, "brown", src, cameraMatrix, k, P, iters)


def _lens_image(who, model, src, K, k, Knew, dsize, flags, dst=None):
    if int(flags) != INTER_LINEAR:
        raise NotImplementedError(f"{who}: INTER_LINEAR only (other interpolations are out of scope)")
    src = np.asarray(src)
    if src.dtype != np.uint8 or not (src.ndim == 2 or (src.ndim == 3 and src.shape[2] in (1, 3))) or 0 in src.shape:
        raise ValueError(f"{who} expects an HxW, HxWx1 or HxWx3 uint8 image")
    fx, fy, cx, cy = _camera_matrix(K, "cameraMatrix")
    fo_x, fo_y, co_x, co_y = (fx, fy, cx, cy) if Knew is None else _camera_matrix(Knew, "newCameraMatrix")
    cam = ofk.camera_setting(model, fx, fy, cx, cy, k, None, fo_x, fo_y, co_x, co_y)
    h, w = src.shape[:2] if dsize is None else (int(dsize[1]), int(dsize[0]))
    if dst is not None and not (isinstance(dst, np.ndarray) and dst.dtype == np.uint8 and dst.shape == (h, w) + src.shape[2:]):
        raise ValueError(f"{who}: dst must be a uint8 array of the result's shape {(h, w) + src.shape[2:]}")
    ctx = ofk.default_context(max(w, src.shape[1]), max(h, src.shape[0]))
    img = src[:, :, 0] if src.ndim == 3 and src.shape[2] == 1 else src
    out = ctx.warp_lens(img, cam, None, (h, w))[0].reshape((h, w) + src.shape[2:])
    if dst is None:
        return out
    dst[...] = out                                               # cv2 fills a dst of the right size and type in place and returns it
    return dst


def undistort(src, cameraMatrix, distCoeffs, dst=None, newCameraMatrix=None, *, flags=INTER_LINEAR):
    """cv2.undistort for HxW or HxWx3 uint8 images: the image rectified into newCameraMatrix (None = cameraMatrix), same size, constant
    border 0 (ofk.h: ofk_warp_lens states the rule; it is the project's, not cv2's block-wise fixed-point map).  4, 5 or 8 distortion
    coefficients; a skewed matrix is refused; a dst of the result's shape and type is filled and returned, any other is refused.  flags
    is not cv2's: it is here to refuse an interpolation other than INTER_LINEAR."""
    k = [] if distCoeffs is None else np.asarray(distCoeffs, np.float64).reshape(-1)
    if len(k) not in (0, 4, 5, 8):
        raise ValueError(f"undistort: {len(k)} distortion coefficients (4, 5 or 8 are supported)")
    return _lens_image("undistort", "brown", src, cameraMatrix, k, newCameraMatrix, None, flags, dst)


class fisheye:
    """cv2.fisheye's point functions and undistortImage (the equidistant model, D = k1..k4)."""

    @staticmethod
    def undistortImage(distorted, K, D, Knew=None, new_size=None, *, flags=INTER_LINEAR):
        """cv2.fisheye.undistortImage: the fisheye image rectified into Knew, new_size = (width, height) (None: the source's).  Knew
        None = K here (cv2's default, the identity matrix, leaves a view one pixel wide).  flags as in undistort."""
        return _lens_image("fisheye.undistortImage", "fisheye", distorted, K, fisheye._d(D, "undistortImage"), Knew, new_size, flags)

    @staticmethod
    def _d(D, who):
        k = np.asarray(D, np.float64).reshape(-1)
        if len(k) != 4:
            raise ValueError(f"fisheye.{who}: D must hold 4 coefficients")
        return k

    @staticmethod
    def undistortPoints(distorted, K, D, R=None, P=None, criteria=None):
        """cv2.fisheye.undistortPoints: pixels -> normalised (or P's) coordinates; 10 Newton steps unless criteria carries a COUNT."""
        _identity_only(R, "fisheye.undistortPoints")
        iters = 10
        if criteria is not None and int(criteria[0]) & TERM_CRITERIA_COUNT:
            iters = int(criteria[1])
        return _lens_points("fisheye.undistortPoints", False, "fisheye", distorted, K, fisheye._d(D, "undistortPoints"), P, iters)

    @staticmethod
    def distortPoints(undistorted, K, D, alpha=0.0):
        """cv2.fisheye.distortPoints: NORMALISED ideal coordinates -> pixels of the fisheye image (alpha, the skew, must be 0)."""
        if alpha != 0.0:
            raise NotImplementedError("fisheye.distortPoints: no skew (alpha)")
        return _lens_points("fisheye.distortPoints", True, "fisheye", undistorted, K, fisheye._d(D, "distortPoints"), None, 10)


class KalmanFilter:
    """cv2.KalmanFilter(dynamParams, measureParams, controlParams) — predict()/correct() run ofk_kf_predict_update.
    Matrices are float64 (the reference assigns float64 numpy arrays, of_module.py:65-76)."""

    def __init__(self, dynamParams, measureParams, controlParams=0, type=None):
        ns, nm, nc = int(dynamParams), int(measureParams), int(controlParams)
        if not (1 <= ns <= 6 and 1 <= nm <= 6 and 0 <= nc <= 6):
            raise ValueError("state/measurement/control sizes up to 6 are supported")
        self._ns, self._nm, self._nc = ns, nm, nc
        self.transitionMatrix = np.eye(ns)
        self.controlMatrix = np.zeros((ns, nc)) if nc else None
        self.measurementMatrix = np.zeros((nm, ns))
        self.processNoiseCov = np.eye(ns)
        self.measurementNoiseCov = np.eye(nm)
        self.statePre = np.zeros((ns, 1)); self.statePost = np.zeros((ns, 1))
        self.errorCovPre = np.zeros((ns, ns)); self.errorCovPost = np.zeros((ns, ns))
        self.gain = np.zeros((ns, nm))

    def _mats(self):
        ns, nm = self._ns, self._nm
        return (np.asarray(self.transitionMatrix, np.float64).reshape(ns, ns),
                np.asarray(self.measurementMatrix, np.float64).reshape(nm, ns),
                np.asarray(self.processNoiseCov, np.float64).reshape(ns, ns),
                np.asarray(self.measurementNoiseCov, np.float64).reshape(nm, nm))

    def predict(self, control=None):
        F, H, Q, R = self._mats()
        ctx = ofk.default_context()
        Bm = u = None
        if control is not None and self.controlMatrix is not None and np.size(self.controlMatrix):
            nc = np.size(control)
            Bm = np.asarray(self.controlMatrix, np.float64).reshape(self._ns, nc); u = np.asarray(control, np.float64).reshape(nc)
        x, P = ctx.kf_predict_update(F, H, Q, R, np.asarray(self.statePost, np.float64).reshape(self._ns),
                                     np.asarray(self.errorCovPost, np.float64).reshape(self._ns, self._ns), B=Bm, u=u, z=None,
                                     do_predict=True)
        self.statePre = x.reshape(-1, 1).copy(); self.errorCovPre = P.copy()
        self.statePost = self.statePre.copy(); self.errorCovPost = self.errorCovPre.copy()
        return self.statePre

    def correct(self, measurement):
        F, H, Q, R = self._mats()
        ctx = ofk.default_context()
        x, P = ctx.kf_predict_update(F, H, Q, R, np.asarray(self.statePre, np.float64).reshape(self._ns),
                                     np.asarray(self.errorCovPre, np.float64).reshape(self._ns, self._ns),
                                     z=np.asarray(measurement, np.float64).reshape(self._nm), do_predict=False)
        self.statePost = x.reshape(-1, 1).copy(); self.errorCovPost = P.copy()
        return self.statePost
