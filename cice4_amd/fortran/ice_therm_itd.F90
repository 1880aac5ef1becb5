!=======================================================================
! Drop-in replacement for the reference's source/ice_therm_itd.F90.
!
! Same module name and public procedures -- linear_itd, add_new_ice, lateral_melt (called from
! source/ice_step_mod.F90:329, 378, 410) with the reference's dummy-argument names -- each forwarding to its
! block-wise entry of the GPU library (include/cice4_amd.h) through cice4_amd_c.  cice_itd_init is made on
! the first call, which is after init_itd.  Nothing of the reference's implementation is kept here.
! The library addresses trcrn as (nx_block,ny_block,max_ntrcr,ncat); the callers hand in the section
! trcrn(:,:,1:ntrcr,:,iblk), which is copied into an array of that shape and back.
!=======================================================================
      module ice_therm_itd

      use ice_kinds_mod
      use ice_domain_size, only: ncat, nilyr, nslyr, ntilyr, ntslyr, max_ntrcr
      use ice_constants
      use ice_fileunits, only: nu_diag
      use iso_c_binding
      use cice4_amd_c

      implicit none
      save
      private
      public :: linear_itd, add_new_ice, lateral_melt

      logical, private :: itd_ready = .false.

      contains

!=======================================================================
      subroutine itd_ensure
      use ice_state, only: ntrcr, trcr_depend, nt_Tsfc, nt_iage, nt_alvl, nt_vlvl
      use ice_age, only: tr_iage
      use ice_mechred, only: tr_lvl
      use ice_flux, only: update_ocn_f
      use ice_itd, only: hin_max, hi_min
      type (cice_itd_config) :: cfg
      if (itd_ready) return
      cfg%ntrcr = ntrcr
      cfg%trcr_depend(:) = 0
      cfg%trcr_depend(1:ntrcr) = trcr_depend(1:ntrcr)
      cfg%nt_Tsfc = nt_Tsfc
      cfg%nt_iage = merge(nt_iage, 0, tr_iage)
      cfg%nt_alvl = merge(nt_alvl, 0, tr_lvl)
      cfg%nt_vlvl = merge(nt_vlvl, 0, tr_lvl)
      cfg%tr_iage = merge(1, 0, tr_iage)
      cfg%tr_lvl = merge(1, 0, tr_lvl)
      cfg%update_ocn_f = merge(1, 0, update_ocn_f)
      cfg%hin_max(1:ncat+1) = hin_max(0:ncat)
      cfg%hi_min = hi_min
      call cice_gpu_ensure()
      call cice_gpu_check(cice_check_sizes(cice_gpu_ctx, ncat, nilyr, nslyr, max_ntrcr), 'ice_therm_itd')
      call cice_gpu_check(cice_itd_init(cice_gpu_ctx, cfg), 'cice_itd_init')
      itd_ready = .true.
      end subroutine itd_ensure

!=======================================================================
      subroutine linear_itd (nx_block,    ny_block,    &
                             icells, indxi, indxj,     &
                             ntrcr,       trcr_depend, &
                             aicen_init,  vicen_init,  &
                             aicen,       trcrn,       &
                             vicen,       vsnon,       &
                             eicen,       esnon,       &
                             aice,        aice0,       &
                             l_stop,                   &
                             istop,       jstop)
      use ice_itd, only: hin_max
      integer (kind=int_kind), intent(in) :: nx_block, ny_block, icells, ntrcr
      integer (kind=int_kind), dimension (nx_block*ny_block), intent(in) :: indxi, indxj
      integer (kind=int_kind), dimension (ntrcr), intent(in) :: trcr_depend
      real (kind=dbl_kind), dimension(nx_block,ny_block,ncat), intent(in) :: aicen_init, vicen_init
      real (kind=dbl_kind), dimension (nx_block,ny_block,ncat), intent(inout) :: aicen, vicen, vsnon
      real (kind=dbl_kind), dimension (nx_block,ny_block,ntrcr,ncat), intent(inout) :: trcrn
      real (kind=dbl_kind), dimension (nx_block,ny_block,ntilyr), intent(inout) :: eicen
      real (kind=dbl_kind), dimension (nx_block,ny_block,ntslyr), intent(inout) :: esnon
      real (kind=dbl_kind), dimension (nx_block,ny_block), intent(inout) :: aice, aice0
      logical (kind=log_kind), intent(out) :: l_stop
      integer (kind=int_kind), intent(out) :: istop, jstop
      real (kind=dbl_kind), allocatable :: tr(:,:,:,:)
      integer (c_int) :: ls
      integer (c_long_long) :: nno

      call itd_ensure
      hin_max(ncat) = 999.9_dbl_kind   ! the reference's side effect (ice_therm_itd.F90:219)
      allocate (tr(nx_block,ny_block,max_ntrcr,ncat))
      tr = c0
      tr(:,:,1:ntrcr,:) = trcrn
      call cice_gpu_check(cice_linear_itd(cice_gpu_ctx, nx_block, ny_block, icells, indxi, indxj, ntrcr, &
         trcr_depend, aicen_init, vicen_init, aicen, tr, vicen, vsnon, eicen, esnon, aice, aice0, ls, istop, &
         jstop, nno), 'linear_itd')
      trcrn = tr(:,:,1:ntrcr,:)
      deallocate (tr)
      l_stop = (ls /= 0)
      if (nno > 0) write(nu_diag,*) 'ITD (GPU): cells not remapped (hicen outside the new boundaries):', nno
      if (l_stop) write(nu_diag,*) 'shift_ice (GPU): daice or dvice out of range at i, j =', istop, jstop
      end subroutine linear_itd

!=======================================================================
      subroutine add_new_ice (nx_block,  ny_block,   &
                              ntrcr,     icells,     &
                              indxi,     indxj,      &
                              tmask,     dt,         &
                              aicen,     trcrn,      &
                              vicen,     eicen,      &
                              aice0,     aice,       &
                              frzmlt,    frazil,     &
                              frz_onset, yday,       &
                              fresh,     fsalt,      &
                              Tf,        l_stop,     &
                              istop,     jstop)
      integer (kind=int_kind), intent(in) :: nx_block, ny_block, ntrcr, icells
      integer (kind=int_kind), dimension (nx_block*ny_block), intent(in) :: indxi, indxj
      logical (kind=log_kind), dimension (nx_block,ny_block), intent(in) :: tmask
      real (kind=dbl_kind), intent(in) :: dt
      real (kind=dbl_kind), dimension (nx_block,ny_block), intent(in) :: aice, frzmlt, Tf
      real (kind=dbl_kind), dimension (nx_block,ny_block,ncat), intent(inout) :: aicen, vicen
      real (kind=dbl_kind), dimension (nx_block,ny_block,ntrcr,ncat), intent(inout) :: trcrn
      real (kind=dbl_kind), dimension (nx_block,ny_block,ntilyr), intent(inout) :: eicen
      real (kind=dbl_kind), dimension (nx_block,ny_block), intent(inout) :: aice0, frazil, fresh, fsalt
      real (kind=dbl_kind), dimension (nx_block,ny_block), intent(inout), optional :: frz_onset
      real (kind=dbl_kind), intent(in), optional :: yday
      logical (kind=log_kind), intent(out) :: l_stop
      integer (kind=int_kind), intent(out) :: istop, jstop
      real (kind=dbl_kind), allocatable :: tr(:,:,:,:), onset(:,:)
      integer (c_int), allocatable :: imask(:,:)
      integer (c_int) :: ls
      real (kind=dbl_kind) :: yd

      call itd_ensure
      allocate (tr(nx_block,ny_block,max_ntrcr,ncat), onset(nx_block,ny_block), imask(nx_block,ny_block))
      tr = c0
      tr(:,:,1:ntrcr,:) = trcrn
      imask = merge(1, 0, tmask)
      ! without both optional arguments nothing is recorded: an onset day that is already set stays
      onset = c1
      yd = c0
      if (present(frz_onset) .and. present(yday)) then
         onset = frz_onset
         yd = yday
      endif
      call cice_gpu_check(cice_add_new_ice(cice_gpu_ctx, nx_block, ny_block, ntrcr, icells, indxi, indxj, imask, &
         dt, aicen, tr, vicen, eicen, aice0, aice, frzmlt, frazil, onset, yd, fresh, fsalt, Tf, ls, istop, jstop), &
         'add_new_ice')
      if (present(frz_onset) .and. present(yday)) frz_onset = onset
      trcrn = tr(:,:,1:ntrcr,:)
      deallocate (tr, onset, imask)
      l_stop = (ls /= 0)
      if (l_stop) write(nu_diag,*) 'Conservation error: vice, add_new_ice (GPU) at i, j =', istop, jstop
      end subroutine add_new_ice

!=======================================================================
      subroutine lateral_melt (nx_block,   ny_block,   &
                               ilo, ihi,   jlo, jhi,   &
                               dt,                     &
                               fresh,      fsalt,      &
                               fhocn,                  &
                               rside,      meltl,      &
                               aicen,      vicen,      &
                               vsnon,      eicen,      &
                               esnon)
      integer (kind=int_kind), intent(in) :: nx_block, ny_block, ilo, ihi, jlo, jhi
      real (kind=dbl_kind), intent(in) :: dt
      real (kind=dbl_kind), dimension (nx_block,ny_block,ncat), intent(inout) :: aicen, vicen, vsnon
      real (kind=dbl_kind), dimension (nx_block,ny_block,ntilyr), intent(inout) :: eicen
      real (kind=dbl_kind), dimension (nx_block,ny_block,ntslyr), intent(inout) :: esnon
      real (kind=dbl_kind), dimension(nx_block,ny_block), intent(in) :: rside
      real (kind=dbl_kind), dimension(nx_block,ny_block), intent(inout) :: fresh, fsalt, fhocn, meltl

      call itd_ensure
      call cice_gpu_check(cice_lateral_melt(cice_gpu_ctx, nx_block, ny_block, ilo, ihi, jlo, jhi, dt, fresh, fsalt, &
         fhocn, rside, meltl, aicen, vicen, vsnon, eicen, esnon), 'lateral_melt')
      end subroutine lateral_melt

!=======================================================================

      end module ice_therm_itd
