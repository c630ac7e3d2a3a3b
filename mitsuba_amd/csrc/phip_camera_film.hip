/*
 * phip_camera_film.hip -- the kernels of phip_camera_rays_device and phip_film_device (k_camera_film.h: k_camera_pixels_check, k_camera_rays, k_film_values) behind
 * the one look-up that returns them (phip_common.h).  One object; phip.hip validates the arguments and launches them (host_camera_film.h).
 */
#include "phip_common.h"
#include "k_camera_film.h"

CameraFilmKernels phipCameraFilmKernels() {
    CameraFilmKernels k;
    k.pixelsCheck = k_camera_pixels_check; k.rays = k_camera_rays;
    k.film[0] = k_film_values<false>; k.film[1] = k_film_values<true>;
    return k;
}
